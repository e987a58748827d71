"""csrc/solve_route.h -- which device calls an iteration of the interior-point loop (program.cc) makes,
as one pure function of seven booleans -- against the table of calls written out independently here, on
the CPU: the header is built into a small shared object with g++ and asked about all 128 inputs.
"""
import ctypes as C
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INPUTS = ("update_mu", "line_search", "quadratic_costs", "timers", "warm_first", "device_mu_supported",
          "triple_supported")
FIELDS = ("mu_on_device", "factor", "mu", "mu_solve_done", "direction", "step", "outcome_read")

# the enumerators of solve_route.h by name: the shim below static_asserts nothing about their values, it
# translates them, so that the header may order them as it likes
SRC = r'''
#include "solve_route.h"
using namespace cxk_route;
static_assert(Choose(Inputs{true, false, false, false, false, true, true}).factor == Factor::kTriple,
              "Choose is a constant expression");
extern "C" void route_choose(const int* in7, int* out7) {
  Inputs in{};
  in.update_mu = in7[0]; in.line_search = in7[1]; in.quadratic_costs = in7[2]; in.timers = in7[3];
  in.warm_first = in7[4]; in.device_mu_supported = in7[5]; in.triple_supported = in7[6];
  const Route r = Choose(in);
  out7[0] = r.mu_on_device;
  switch (r.factor) {
    case Factor::kTriple: out7[1] = 0; break;
    case Factor::kSolve: out7[1] = 1; break;
    case Factor::kDirection: out7[1] = 2; break;
    case Factor::kPlain: out7[1] = 3; break;
  }
  switch (r.mu) {
    case Mu::kDevice: out7[2] = 0; break;
    case Mu::kHost: out7[2] = 1; break;
    case Mu::kKept: out7[2] = 2; break;
  }
  out7[3] = r.mu_solve_done;
  switch (r.direction) {
    case Direction::kDeviceMu: out7[4] = 0; break;
    case Direction::kNone: out7[4] = 1; break;
    case Direction::kHost: out7[4] = 2; break;
  }
  switch (r.step) {
    case Step::kPrepareTakeDeviceMu: out7[5] = 0; break;
    case Step::kPrepareTake: out7[5] = 1; break;
    case Step::kPrepare: out7[5] = 2; break;
  }
  switch (r.outcome_read) {
    case OutcomeRead::kAfterMuSelection: out7[6] = 0; break;
    case OutcomeRead::kAfterPrepare: out7[6] = 1; break;
  }
}
'''
FACTOR = ("triple", "factor_solve", "factor_direction", "factor")
MU = ("device", "host", "kept")
DIRECTION = ("device_mu", "none", "newton_direction")
STEP = ("prepare_take_step_device_mu", "prepare_take_step", "prepare_step")
OUTCOME_READ = ("after_mu_selection", "after_prepare")


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    """{inputs (7 bools): route (dict)} for all 128 inputs, as the header answers."""
    d = tmp_path_factory.mktemp("solve_route")
    src = d / "solve_route_test.cc"
    src.write_text(SRC)
    so = d / "libsolve_route_test.so"
    # a bare g++: no HIP, nothing else of the project on the include path's other headers is needed
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "conex_amd", "csrc"), str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.route_choose.restype = None
    lib.route_choose.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    out = {}
    for bits in itertools.product((False, True), repeat=7):
        a = (C.c_int * 7)(*[int(b) for b in bits])
        r = (C.c_int * 7)(*([-1] * 7))
        lib.route_choose(a, r)
        out[bits] = dict(mu_on_device=bool(r[0]), factor=FACTOR[r[1]], mu=MU[r[2]], mu_solve_done=bool(r[3]),
                         direction=DIRECTION[r[4]], step=STEP[r[5]], outcome_read=OUTCOME_READ[r[6]])
    assert len(out) == 128
    return out


def table(update_mu, line_search, quadratic_costs, timers, warm_first, device_mu_supported, triple_supported):
    """The route as the loop has always taken it, one row of the table per field."""
    mu_on_device = (update_mu and not line_search and not quadratic_costs and not timers and not warm_first
                    and device_mu_supported)
    if mu_on_device and triple_supported:
        factor = "triple"
    elif update_mu and not line_search:
        factor = "factor_solve"
    elif not update_mu:
        factor = "factor_direction"
    else:
        factor = "factor"
    mu = "device" if mu_on_device else "host" if update_mu else "kept"
    direction = "device_mu" if mu_on_device else "none" if not update_mu else "newton_direction"
    if mu_on_device:
        step = "prepare_take_step_device_mu"
    elif update_mu and not warm_first:
        step = "prepare_take_step"
    else:
        step = "prepare_step"
    outcome_read = "after_mu_selection" if update_mu and not mu_on_device else "after_prepare"
    return dict(mu_on_device=mu_on_device, factor=factor, mu=mu, mu_solve_done=update_mu and not line_search,
                direction=direction, step=step, outcome_read=outcome_read)


def test_every_field_matches_the_table_for_all_128_inputs(routes):
    for bits, got in routes.items():
        want = table(*bits)
        assert set(got) == set(FIELDS) == set(want)
        for f in FIELDS:
            assert got[f] == want[f], (dict(zip(INPUTS, bits)), f, got[f], want[f])


def test_every_call_of_every_field_is_reached(routes):
    for f, names in (("factor", FACTOR), ("mu", MU), ("direction", DIRECTION), ("step", STEP),
                     ("outcome_read", OUTCOME_READ)):
        assert {r[f] for r in routes.values()} == set(names), f


def test_invariants_of_the_table(routes):
    for bits, r in routes.items():
        i = dict(zip(INPUTS, bits))
        # the outcome is read in exactly one place: behind the host's selection exactly when the host selects,
        # which is the first host round trip of the iteration then; behind PrepareStep otherwise
        assert r["outcome_read"] in OUTCOME_READ
        assert (r["outcome_read"] == "after_mu_selection") == (r["mu"] == "host"), i
        # the three right-hand sides only for a barrier parameter selected on the device
        if r["factor"] == "triple":
            assert r["mu_on_device"], i
        assert r["mu_on_device"] == (r["mu"] == "device") == (r["direction"] == "device_mu") \
            == (r["step"] == "prepare_take_step_device_mu"), i
        # no direction call exactly when the direction rode in the factor sweep
        assert (r["direction"] == "none") == (r["factor"] == "factor_direction"), i
        # PrepareStep alone, TakeStep from the host afterwards
        assert (r["step"] == "prepare_step") == (not i["update_mu"] or (i["warm_first"] and not r["mu_on_device"])), i
        # the solve of the host's selection came with the factorization exactly when that call carried it
        # (or the three that contain it)
        assert r["mu_solve_done"] == (r["factor"] in ("triple", "factor_solve")), i


def test_the_header_includes_nothing():
    """No HIP, no I/O, no allocation: nothing to do any of them with."""
    with open(os.path.join(ROOT, "conex_amd", "csrc", "solve_route.h")) as f:
        assert "#include" not in f.read()
