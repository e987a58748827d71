"""A program whose quadratic cone has its matrix given by its nonzeros, end to end through
Conex.AddSparseQuadraticConstraint: risk-bounded return maximisation over 300 assets,

    max mu' x   s.t.   sqrt(x' Q x) <= t,  t <= RISK,  sum x <= 1,  0 <= x <= CAP,

over y = (x, t).  The cone is c - A y = (t, x): A0 = -e_t, A1 = -[I 0], a selection; Q = D + F Sigma F' is a factor
model.  Solved once with AddSparseQuadraticConstraint and once with AddStructuredQuadraticConstraint (or, with a dense
Q, AddQuadraticConstraint) on the expanded A: the two solutions agree to RESTATED_TOLERANCE, the tolerance
test_gpu_quad_structured_solve.py uses for its restatement comparison, and the iteration counts are equal or differ
by one.
"""
import numpy as np
import pytest

from conex_amd.program import Conex
from test_gpu_quad_structured_solve import RESTATED_TOLERANCE, diagonal_csr

pytestmark = pytest.mark.gpu

ASSETS, FACTORS = 300, 5
RISK, CAP = 0.08, 0.02


def portfolio_data():
    rng = np.random.default_rng(33)
    n = ASSETS
    D = rng.uniform(0.01, 0.04, n)
    F = rng.uniform(0.0, 0.3, (n, FACTORS))
    sigma = rng.uniform(0.5, 1.5, FACTORS)
    mu = rng.uniform(0.0, 0.1, n)
    m = n + 1
    A = np.zeros((n + 1, m))
    A[0, n] = -1.0
    A[1 + np.arange(n), np.arange(n)] = -1.0
    c = np.zeros(n + 1)
    # budget, risk bound and the box as linear inequalities c - A y >= 0
    L = np.zeros((2 + 2 * n, m))
    lc = np.zeros(2 + 2 * n)
    L[0, :n], lc[0] = 1.0, 1.0
    L[1, n], lc[1] = 1.0, RISK
    L[2 + np.arange(n), np.arange(n)], lc[2:2 + n] = 1.0, CAP
    L[2 + n + np.arange(n), np.arange(n)] = -1.0
    cost = np.r_[mu, 0.0]
    return D, F, sigma, A, c, L, lc, cost


def csr_of(A):
    mask = A != 0
    rows, cols = np.nonzero(mask)
    return np.r_[0, np.cumsum(mask.sum(axis=1))].astype(np.int32), cols.astype(np.int32), A[rows, cols].copy()


def solve(add_cone):
    D, F, sigma, A, c, L, lc, cost = portfolio_data()
    p = Conex(ASSETS + 1)
    assert add_cone(p, D, F, sigma, A, c) == 0
    p.AddLinearInequality(L, lc)
    assert p.num_constraints == 2
    cfg = p.DefaultConfiguration()
    sol = p.Maximize(cost, cfg)
    assert sol.status == 1
    return sol, len(p.GetIterationStats())


@pytest.mark.parametrize("q_form", ["parts", "dense"])
def test_risk_bounded_return_maximisation_by_nonzeros_equals_the_expanded_form(q_form):
    def sparse(p, D, F, sigma, A, c):
        Q = dict(S=diagonal_csr(D), F=F, sigma=sigma) if q_form == "parts" else np.diag(D) + (F * sigma) @ F.T
        return p.AddSparseQuadraticConstraint(Q, csr_of(A), c)

    def expanded(p, D, F, sigma, A, c):
        if q_form == "parts":
            return p.AddStructuredQuadraticConstraint(diagonal_csr(D), F, sigma, A, c)
        return p.AddQuadraticConstraint(np.diag(D) + (F * sigma) @ F.T, A, c)

    a, iters_a = solve(sparse)
    b, iters_b = solve(expanded)
    print(f"by nonzeros against expanded: {np.linalg.norm(a.y - b.y):.3g}; iterations {iters_a} / {iters_b}")
    assert np.linalg.norm(a.y - b.y) <= RESTATED_TOLERANCE
    assert abs(iters_a - iters_b) <= 1
    # the solution is one: the risk bound or the budget binds, the box holds
    x, t = a.y[:ASSETS], a.y[ASSETS]
    D, F, sigma = portfolio_data()[:3]
    risk = float(np.sqrt(x @ (D * x + F @ (sigma * (F.T @ x)))))
    assert risk <= t + 1e-6 and t <= RISK + 1e-6 and np.sum(x) <= 1 + 1e-6 and np.all(x >= -1e-6) and np.all(x <= CAP + 1e-6)
    assert RISK - t <= 1e-3 or 1 - np.sum(x) <= 1e-3
