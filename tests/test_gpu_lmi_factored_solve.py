"""Programs whose matrix inequality is given by factors, end to end through Conex.AddFactoredLinearMatrixInequality,
against the oracle on the expanded matrices.

E-optimal design: n = 12, 40 candidate vectors a_i; maximize t subject to sum_i lambda_i a_i a_i' - t I >= 0,
lambda >= 0, sum lambda <= 1.  Over y = (lambda, t) the matrix constraint is 0 - sum_i y_i A_i >= 0 with
A_i = -a_i a_i' (rank one, sigma = -1) and A_t = I (rank 12, columns e_k); the bounds are linear rows.
Rank-one program: n = 30, m = 45, C - sum_i y_i a_i a_i' >= 0 with C > 0 and b_i = a_i' X0 a_i for X0 > 0 (strictly
feasible on both sides, synthetic.factored_lmi_problem); at the optimum a_i' X a_i = b_i.

Status and y are the oracle's (rtol 1e-6, atol 1e-8: the tolerance of test_gpu_soc_sparse_solve.py).  The iteration
count is the oracle's, or off by one: the factored route's W differs from the expanded route's in the last bits, and
an iteration whose stopping measure sits at its threshold then falls on either side (DESIGN.md 8.4 records the same
for C4).
"""
import numpy as np
import pytest

import oracle_lib as ol
from conex_amd import synthetic as syn
from conex_amd.program import Conex

pytestmark = pytest.mark.gpu


def design_data():
    rng = np.random.default_rng(2031)
    n, cand = 12, 40
    a = rng.standard_normal((n, cand))
    F = np.hstack([a, np.eye(n)])
    rank_ptr = np.r_[np.arange(cand + 1), cand + n]
    sigma = np.r_[-np.ones(cand), np.ones(n)]
    Lin = np.vstack([np.hstack([-np.eye(cand), np.zeros((cand, 1))]), np.r_[np.ones(cand), 0.0][None]])
    lin_c = np.r_[np.zeros(cand), 1.0]
    cost = np.r_[np.zeros(cand), 1.0]
    return n, cand, a, F, rank_ptr, sigma, Lin, lin_c, cost


def build_design():
    n, cand, a, F, rank_ptr, sigma, Lin, lin_c, cost = design_data()
    p = Conex(cand + 1)
    assert p.AddFactoredLinearMatrixInequality(F, rank_ptr, sigma, np.zeros((n, n))) == 0
    p.AddLinearInequality(Lin, lin_c)
    o = ol.Program(cand + 1)
    assert o.add_lmi(syn.expand_factors(F, rank_ptr, sigma), np.zeros((n, n))) == 0
    assert o.add_linear(Lin, lin_c) == 1
    return p, o, cost


def build_rank_one():
    prob = syn.factored_lmi_problem(K=1, n=30, ranks=(1,) * 45, seed=2032)
    p = Conex(45)
    assert p.AddFactoredLinearMatrixInequality(prob["F"][0], prob["rank_ptr"][0], prob["sigma"][0], prob["C"][0]) == 0
    o = ol.Program(45)
    assert o.add_lmi(prob["A"][0], prob["C"][0]) == 0
    return p, o, prob["b"], prob


def solve_both(p, o, cost):
    cfg = p.DefaultConfiguration()
    sol = p.Maximize(cost, cfg)
    ocfg = ol.default_config()
    for f, _ in ocfg._fields_:
        setattr(ocfg, f, getattr(cfg, f))
    oko, yo = o.solve(cost, ocfg)
    iters, iters_o = p.GetIterationNumberStats(-1).iteration_number + 1, o.num_iterations()
    print(f"status {sol.status} / {oko}, iterations {iters} / {iters_o}, |y - yo| {np.max(np.abs(sol.y - yo)):.3g}")
    assert sol.status == oko == 1
    assert np.allclose(sol.y, yo, rtol=1e-6, atol=1e-8)
    assert abs(iters - iters_o) <= 1  # (see the module's docstring)
    return sol, yo


def test_e_optimal_design_matches_the_oracle():
    p, o, cost = build_design()
    sol, yo = solve_both(p, o, cost)
    n, cand, a = design_data()[:3]
    lam, t = sol.y[:cand], sol.y[cand]
    assert lam.min() >= -1e-8 and lam.sum() <= 1 + 1e-8
    # t is the smallest eigenvalue of the information matrix, to the solve's tolerance
    assert abs(np.linalg.eigvalsh((a * lam) @ a.T).min() - t) <= 1e-5
    X = p.GetDualVariables()[0]
    assert X.shape == (n, n) and np.linalg.eigvalsh(0.5 * (X + X.T)).min() >= -1e-9
    assert abs(np.trace(X) - 1.0) <= 1e-5  # the multiplier of t


def test_rank_one_program_matches_the_oracle_and_its_dual_reproduces_b():
    p, o, b, prob = build_rank_one()
    sol, _ = solve_both(p, o, b)
    X = p.GetDualVariables()[0]
    _, err = p.ComputeErrors(sol.y, [X], b)  # (the operator and its adjoint from the factors)
    assert err.Ax_minus_b <= 1e-5 * max(1.0, np.abs(b).max()) and err.min_eig_S[0] >= -1e-9
    assert X.shape == (30, 30) and np.allclose(X, X.T, atol=1e-9 * np.abs(X).max())
    assert np.linalg.eigvalsh(0.5 * (X + X.T)).min() >= -1e-9
    F = prob["F"][0]
    got = np.einsum("ak,ab,bk->k", F, X, F)
    # (1e-5: what test_python_frontend.py asks of |b - A^* x| after a solve at the default options)
    assert np.max(np.abs(got - b)) <= 1e-5 * max(1.0, np.abs(b).max()), np.max(np.abs(got - b))


def test_a_warm_started_resolve_converges():
    p, o, cost = build_design()
    cfg = p.DefaultConfiguration()
    cold = p.Maximize(cost, cfg)
    assert cold.status == 1
    cfg.initialization_mode = 1
    warm = p.Maximize(cost, cfg)
    assert warm.status == 1
    assert np.allclose(warm.y, cold.y, rtol=1e-5, atol=1e-7)
