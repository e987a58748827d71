"""A sparse least-squares program end to end through conex.h with its cone on the sparse route.

min t  s.t.  |A x - b| <= t  with 400 rows, 60 unknowns and 3 nonzeros per row of A, built entry by entry through the
Python Conex class (CONEX_NewLorentzConeConstraint makes the cone as wide as the program, 401 x 61) with
CONEX_HIP_SetSparseSoc(program, 1): the program layer hands the device its dense host copy, the device reads the
nonzeros off it.  A second, small cone (|x[:3]| <= 10, inactive at the optimum) rides along, as in
test_gpu_soc_streamed_solve.py.
"""
import numpy as np
import pytest

import oracle_lib as ol
from conex_amd.program import Conex

ROWS, UNKNOWNS, PER_ROW = 400, 60, 3
# |x - lstsq| / |lstsq| of the ORACLE's solve of this program at the default options: 1.92e-8 measured on the CPU (x
# is the minimiser at every t on the central path; what is left is the last Newton step's); the test allows ten times that.
X_VS_LSTSQ_ORACLE = 1.9e-8


def least_squares_data():
    rng = np.random.default_rng(2030)
    A = np.zeros((ROWS, UNKNOWNS))
    for r in range(ROWS):
        pick = rng.choice(UNKNOWNS, size=PER_ROW, replace=False)
        A[r, pick] = rng.uniform(-1, 1, PER_ROW)
    b = rng.uniform(-1, 1, ROWS)
    return A, b


def cone_data():
    """(M, c) of the two cones over y = (x, t): c - M y = (t, A x - b) and (10, x[:3])."""
    A, b = least_squares_data()
    m = UNKNOWNS + 1
    M1 = np.zeros((ROWS + 1, m))
    M1[0, UNKNOWNS] = -1.0
    M1[1:, :UNKNOWNS] = -A
    c1 = np.r_[0.0, -b]
    M2 = np.zeros((4, m))
    M2[1:, :3] = -np.eye(3)
    c2 = np.r_[10.0, np.zeros(3)]
    cost = np.zeros(m)
    cost[UNKNOWNS] = -1.0  # maximize -t
    return (M1, c1), (M2, c2), cost


def build_program(sparse=None):
    (M1, c1), (M2, c2), cost = cone_data()
    p = Conex(UNKNOWNS + 1)
    if sparse is not None:
        assert p._L.CONEX_HIP_SetSparseSoc(p.a, int(sparse)) == 0
    for M, c in ((M1, c1), (M2, c2)):
        cid = p.NewLorentzConeConstraint(M.shape[0] - 1)
        for r, j in zip(*np.nonzero(M)):
            p.UpdateLinearOperator(cid, M[r, j], int(j), int(r))
        for r in np.nonzero(c)[0]:
            p.UpdateAffineTerm(cid, c[r], int(r))
    return p, cost


def oracle_solve(cfg):
    (M1, c1), (M2, c2), cost = cone_data()
    o = ol.Program(UNKNOWNS + 1)
    o.add_soc(M1, c1)
    o.add_soc(M2, c2)
    ocfg = ol.default_config()
    for f, _ in ocfg._fields_:
        setattr(ocfg, f, getattr(cfg, f))
    ok, y = o.solve(cost, ocfg)
    return ok, y, o.num_iterations()


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.gpu
def test_sparse_least_squares_on_the_sparse_route_matches_the_oracle_and_lstsq():
    """y and the iteration count are the oracle's (the tolerance of test_gpu_solver.py's second-order cone solve); x
    is numpy.linalg.lstsq's to ten times what the oracle's own answer achieves, X_VS_LSTSQ_ORACLE (asserted here to be
    what the oracle still achieves, within a factor of two)."""
    A, b = least_squares_data()
    x_ls = np.linalg.lstsq(A, b, rcond=None)[0]
    p, cost = build_program(sparse=1)
    assert p._L.CONEX_HIP_CountSparseSoc(p.a) == -1  # no device context yet
    cfg = p.DefaultConfiguration()
    sol = p.Maximize(cost, cfg)
    oko, yo, iters = oracle_solve(cfg)
    assert oko == 1 and sol.status == 1
    assert p._L.CONEX_HIP_CountSparseSoc(p.a) == 2  # mode 1: both cones
    assert np.allclose(sol.y, yo, rtol=1e-6, atol=1e-8)
    assert p.GetIterationNumberStats(-1).iteration_number == iters - 1
    measured = rel(yo[:UNKNOWNS], x_ls)
    print(f"oracle x against lstsq: {measured:.3g}; device x against lstsq: {rel(sol.y[:UNKNOWNS], x_ls):.3g}")
    assert 0.5 * X_VS_LSTSQ_ORACLE <= measured <= 2 * X_VS_LSTSQ_ORACLE, measured
    assert rel(sol.y[:UNKNOWNS], x_ls) <= 10 * X_VS_LSTSQ_ORACLE


@pytest.mark.gpu
def test_warm_started_resolve_on_the_sparse_route():
    """initialization_mode = 1 continues from the device's scaling points: get_W / set_W of a sparse cone."""
    p, cost = build_program(sparse=1)
    cfg = p.DefaultConfiguration()
    cold = p.Maximize(cost, cfg)
    assert cold.status == 1
    cfg.initialization_mode = 1
    warm = p.Maximize(cost, cfg)
    assert warm.status == 1
    assert p._L.CONEX_HIP_CountSparseSoc(p.a) == 2


@pytest.mark.gpu
def test_without_the_call_the_program_counts_no_sparse_cones():
    """The default of conex.h programs is mode 0: the same program keeps the streamed and the staged kernels."""
    p, cost = build_program()
    sol = p.Maximize(cost, p.DefaultConfiguration())
    assert sol.status == 1
    assert p._L.CONEX_HIP_CountSparseSoc(p.a) == 0
