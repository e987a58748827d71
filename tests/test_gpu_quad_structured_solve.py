"""Programs whose quadratic cone has Q = S + F diag(sigma) F' given by its parts, end to end through
Conex.AddStructuredQuadraticConstraint.

(a) A norm ball: max b'y s.t. y'Qy <= 1 with 300 variables and Q = D + F1 F1' - rho f f' (the one test with a negative
    sigma; |f| = 1 and rho = min(D) / 2, so Q >= D - rho I > 0 by construction); the optimum is
    y* = Q^{-1} b / sqrt(b' Q^{-1} b), from the expanded Q.  Bounds: those of test_gpu_quad_streamed_solve.py.
(b) Generalised least squares: min t s.t. |A x - b|_Q <= t with 50 000 rows (beyond the dense form: n^2 > 2^31) and 3
    unknowns, Q = D + F F' (diagonal plus rank 2), default options.  The same program restated as a cone without Q over
    the stacked rows [D^{1/2}; F'] (A x - b), through the existing AddQuadraticConstraint(None, ...), is the reference:
    the two solutions differ by at most 8e-6 in norm (the reference's own tolerance for this equivalence,
    test_quadratic_cone.py), and t is within the central path's gap 2 mu = 2e-6 of sqrt(r' Q r) at the closed-form
    minimiser.
(c) A warm-started re-solve of (b).
"""
import numpy as np
import pytest

import oracle_lib as ol
from conex_amd.program import Conex
from test_gpu_quad_streamed_solve import T_VS_LSTSQ, copy_config

pytestmark = pytest.mark.gpu

BALL_N = 300
ROWS, UNKNOWNS = 50_000, 3
RESTATED_TOLERANCE = 8e-6


def diagonal_csr(d):
    n = len(d)
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.asarray(d, dtype=np.float64)


# ------------------------------------------------------------------------------------ (a) the norm ball
def ball_data():
    rng = np.random.default_rng(21)
    n = BALL_N
    D = rng.uniform(1.0, 2.0, n)
    F1 = rng.uniform(-1, 1, (n, 3)) / np.sqrt(n)
    f = rng.uniform(-1, 1, n)
    f /= np.linalg.norm(f)
    rho = 0.5 * float(np.min(D))
    F = np.column_stack([F1, f])
    sigma = np.array([1.0, 1.0, 1.0, -rho])
    Q = np.diag(D) + (F * sigma) @ F.T
    assert np.min(np.linalg.eigvalsh(Q)) >= np.min(D) - rho - 1e-12 > 0
    b = rng.uniform(-1, 1, n)
    A = np.vstack([np.zeros((1, n)), -np.eye(n)])  # c - A y = (1, y)
    c = np.r_[1.0, np.zeros(n)]
    return diagonal_csr(D), F, sigma, Q, A, c, b


def test_norm_ball_with_a_negative_sigma_matches_the_closed_form_and_the_oracle():
    S, F, sigma, Q, A, c, b = ball_data()
    p = Conex(BALL_N)
    assert p.AddStructuredQuadraticConstraint(S, F, sigma, A, c) == 0
    cfg = p.DefaultConfiguration()
    cfg.inv_sqrt_mu_max = 1e4
    cfg.max_iterations = 50
    sol = p.Maximize(b, cfg)
    assert sol.status == 1
    z = np.linalg.solve(Q, b)
    y_star = z / np.sqrt(b @ z)
    print(f"device y against the closed form: {np.linalg.norm(sol.y - y_star):.3g}")
    assert np.linalg.norm(sol.y - y_star) <= 1e-4 * (1 + np.linalg.norm(y_star))
    o = ol.Program(BALL_N)
    assert o.add_quadratic(Q, A, c) == 0
    oko, yo = o.solve(b, copy_config(cfg))
    assert oko == 1
    print(f"device y against the oracle: {np.max(np.abs(sol.y - yo)):.3g}")
    assert np.allclose(sol.y, yo, rtol=1e-6, atol=1e-8)


# ------------------------------------------------------------------------------------ (b) generalised least squares
def gls_data():
    rng = np.random.default_rng(22)
    A = rng.uniform(-1, 1, (ROWS, UNKNOWNS))
    b = rng.uniform(-1, 1, ROWS)
    D = rng.uniform(1.0, 2.0, ROWS)
    F = rng.uniform(0.0, 1.0, (ROWS, 2)) / np.sqrt(ROWS)
    return A, b, D, F


def apply_q(D, F, X):
    return D[:, None] * X + F @ (F.T @ X) if X.ndim == 2 else D * X + F @ (F.T @ X)


def cone_data(rows_of):
    """(M, c) of the cone over y = (x, t): c - M y = (t, L (A x - b)) for the row map L, and the cost (maximize -t)."""
    A, b, D, F = gls_data()
    LA, Lb = rows_of(A, D, F), rows_of(b, D, F)
    m = UNKNOWNS + 1
    M = np.zeros((LA.shape[0] + 1, m))
    M[0, UNKNOWNS] = -1.0
    M[1:, :UNKNOWNS] = -LA
    cost = np.zeros(m)
    cost[UNKNOWNS] = -1.0
    return M, np.r_[0.0, -Lb], cost


def identity_rows(X, D, F):
    return X


def stacked_rows(X, D, F):
    """[D^{1/2}; F'] X: |L r|^2 = r' (D + F F') r."""
    return np.concatenate([(np.sqrt(D) * X.T).T, F.T @ X], axis=0)


def structured_program():
    A, b, D, F = gls_data()
    M, c, cost = cone_data(identity_rows)
    p = Conex(UNKNOWNS + 1)
    assert p.AddStructuredQuadraticConstraint(diagonal_csr(D), F, None, M, c) == 0
    return p, cost


def test_generalised_least_squares_beyond_the_dense_form_matches_its_restatement_and_the_closed_form():
    assert ROWS * ROWS > 2 ** 31 - 1
    A, b, D, F = gls_data()
    p, cost = structured_program()
    cfg = p.DefaultConfiguration()
    sol = p.Maximize(cost, cfg)
    assert sol.status == 1
    # the restated program: a cone without Q over ROWS + 2 rows, on the existing route
    M, c, _ = cone_data(stacked_rows)
    q = Conex(UNKNOWNS + 1)
    assert q.AddQuadraticConstraint(None, M, c) == 0
    restated = q.Maximize(cost, q.DefaultConfiguration())
    assert restated.status == 1
    print(f"structured against restated: {np.linalg.norm(sol.y - restated.y):.3g}")
    assert np.linalg.norm(sol.y - restated.y) <= RESTATED_TOLERANCE
    # the closed-form minimiser of (A x - b)' Q (A x - b)
    QA, Qb = apply_q(D, F, A), apply_q(D, F, b)
    x_star = np.linalg.solve(A.T @ QA, A.T @ Qb)
    r = A @ x_star - b
    t_star = float(np.sqrt(r @ apply_q(D, F, r)))
    print(f"t against the closed form: {abs(sol.y[UNKNOWNS] - t_star):.3g}")
    assert abs(sol.y[UNKNOWNS] - t_star) <= T_VS_LSTSQ


def test_warm_started_resolve_of_a_structured_quadratic_cone():
    p, cost = structured_program()
    cfg = p.DefaultConfiguration()
    cold = p.Maximize(cost, cfg)
    assert cold.status == 1
    cfg.initialization_mode = 1
    warm = p.Maximize(cost, cfg)
    assert warm.status == 1
