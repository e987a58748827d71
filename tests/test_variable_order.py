"""Vectors in the original variable order are indexed by variable (include/conex_kkt_hip.h above cxk_solve_inplace):
cxk_get_y, cxk_set_y, cxk_solve_inplace, cxk_get_residuals and cxk_get_valid_variables address entry
permutation_inverse[p] for every eliminated position p < N, and N counts only the variables that occur in a
constraint.  A context that leaves variables out therefore needs vectors longer than N: the binding sizes them by
KktContext.span (one entry per variable and multiplier), and refuses shorter input.

cxk_get_valid_variables needs no device, so the C entry point itself runs here on host-only contexts: the mask has
span entries, exactly the variables in use are set, and the bytes behind the mask's end are left alone."""
import ctypes as C

import numpy as np
import pytest

from conex_amd import KktContext
from conex_amd import synthetic as syn

NUM_VARS = 64


def soc_over(variables, rows=4):
    """One second-order cone over `variables` of a 64-variable context (the shape of a constraint alone on its route
    in test_gpu_every_route.py)."""
    rng = np.random.default_rng(len(variables))
    c = np.zeros(rows)
    c[0] = 1.0
    k = KktContext(NUM_VARS, device=-1)
    assert k.add_soc(rng.uniform(-1, 1, (rows, len(variables))), c, list(variables)) == 0
    k.initialize()
    return k


GAPS = [[1, 2], list(range(2, 64)), [12, 13, 14], [0, 63], [0, 1]]


@pytest.mark.parametrize("used", GAPS, ids=lambda u: f"{u[0]}-{u[-1]}x{len(u)}")
def test_valid_variables_is_indexed_by_variable(used):
    k = soc_over(used)
    assert k.N == len(used) and k.span == NUM_VARS
    mask = k.valid_variables()
    assert mask.shape == (NUM_VARS,)
    assert np.array_equal(np.flatnonzero(mask), used)
    # the C entry point on a buffer of span entries with a guard behind it: the guard survives, and with only N
    # entries in front of it (what the binding used to allocate) it would not where the largest variable is >= N
    guard = 0xA5
    buf = np.full(k.span + 16, guard, dtype=np.uint8)
    assert k.L.cxk_get_valid_variables(k.h, buf.ctypes.data_as(C.POINTER(C.c_ubyte))) == 0
    assert np.all(buf[k.span:] == guard)
    assert np.array_equal(np.flatnonzero(buf[:k.span] == 1), used)
    assert np.all(buf[:k.span][np.setdiff1d(np.arange(k.span), used)] == guard)  # unused entries are not written
    assert (max(used) >= k.N) == (used != [0, 1])


def test_multipliers_follow_the_variables():
    k = KktContext(6, device=-1)
    k.add_linear(np.ones((3, 2)), np.ones(3), [1, 4])
    k.add_equality(np.ones((2, 2)), np.zeros(2), [1, 4])
    k.initialize()
    assert k.N == 2 + 2 and k.span == 6 + 2
    assert np.array_equal(np.flatnonzero(k.valid_variables()), [1, 4, 6, 7])


@pytest.mark.parametrize("kind,prob", [("lmi", syn.lmi_problem(K=9, n=4, m=6, branching=2, overlap=2)),
                                       ("soc", syn.soc_problem(K=7, dim=3, m=5, overlap=2)),
                                       ("lp", syn.lp_problem(rows=8, num_vars=5))])
def test_every_variable_in_use_means_span_is_n(kind, prob):
    k = syn.build(KktContext, prob, kind, device=-1)
    assert k.span == k.N == k.num_vars
    assert k.valid_variables().all()


def test_shorter_input_is_refused_before_it_reaches_the_library():
    k = soc_over(list(range(2, 64)))
    assert k.N == 62
    for call in (k.set_y, k.solve_inplace, lambda y: k.prepare_step(y, 1.0), lambda y: k.weighted_slack_eigenvalues(y, 1.0)):
        with pytest.raises(ValueError, match="64 entries"):
            call(np.zeros(k.N))  # N entries: what fits a context without unused variables
