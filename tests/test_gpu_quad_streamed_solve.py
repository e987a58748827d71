"""Programs whose quadratic cone runs on the streamed kernels, end to end through Conex.AddQuadraticConstraint.

(a) A norm ball: max b'y s.t. y'Qy <= 1 with 300 variables and a dense Q, every cone on the streamed route
    (CONEX_HIP_SetStreamedQuadratic(program, 1)); the optimum is y* = Q^{-1} b / sqrt(b' Q^{-1} b).
(b) Least squares: min t s.t. |A x - b| <= t with 5200 rows and 3 unknowns as a quadratic cone without Q, whose
    4 + 4 * 5201 = 20 808 doubles are beyond the LDS kernels -- the program layer's default (automatic) takes the
    streamed route, so the solve needs no new call.
"""
import numpy as np
import pytest

import oracle_lib as ol
from conex_amd.program import Conex

pytestmark = pytest.mark.gpu

BALL_N = 300
ROWS, UNKNOWNS = 5200, 3
# |x - lstsq| / |lstsq| of the ORACLE's solve of program (b) at the default options: 4.0e-15 measured (x is the
# minimiser at every t on the central path, and with three unknowns the last Newton step leaves rounding only); the
# test allows ten times that and asserts that the oracle still achieves it within a factor of two.
X_VS_LSTSQ_ORACLE = 4.0e-15
# t against lstsq's residual norm: the cone has rank 2, so on the central path the gap is 2 mu, and the default
# options stop at mu = 1 / inv_sqrt_mu_max^2 = 1e-6 (the oracle: 1.0e-6 measured, 2.4e-8 of t).
T_VS_LSTSQ = 2 * 1e-6


def copy_config(cfg):
    ocfg = ol.default_config()
    for f, _ in ocfg._fields_:
        setattr(ocfg, f, getattr(cfg, f))
    return ocfg


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ------------------------------------------------------------------------------------ (a) the norm ball
def ball_data():
    rng = np.random.default_rng(11)
    n = BALL_N
    R = rng.uniform(-1, 1, (n, n))
    Q = R @ R.T / n + np.eye(n)
    b = rng.uniform(-1, 1, n)
    A = np.vstack([np.zeros((1, n)), -np.eye(n)])  # c - A y = (1, y)
    c = np.r_[1.0, np.zeros(n)]
    return Q, A, c, b


def test_norm_ball_on_the_streamed_route_matches_the_closed_form_and_the_oracle():
    Q, A, c, b = ball_data()
    p = Conex(BALL_N)
    assert p._L.CONEX_HIP_SetStreamedQuadratic(p.a, 1) == 0
    assert p.AddQuadraticConstraint(Q, A, c) == 0
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
    assert np.allclose(sol.y, yo, rtol=1e-6, atol=1e-8)


# ------------------------------------------------------------------------------------ (b) least squares
def least_squares_data():
    rng = np.random.default_rng(12)
    A = rng.uniform(-1, 1, (ROWS, UNKNOWNS))
    b = rng.uniform(-1, 1, ROWS)
    return A, b


def cone_data():
    """(M, c) of the cone over y = (x, t): c - M y = (t, A x - b), and the cost (maximize -t)."""
    A, b = least_squares_data()
    m = UNKNOWNS + 1
    M = np.zeros((ROWS + 1, m))
    M[0, UNKNOWNS] = -1.0
    M[1:, :UNKNOWNS] = -A
    cost = np.zeros(m)
    cost[UNKNOWNS] = -1.0
    return M, np.r_[0.0, -b], cost


def build_program(mode=None):
    M, c, cost = cone_data()
    p = Conex(UNKNOWNS + 1)
    if mode is not None:
        assert p._L.CONEX_HIP_SetStreamedQuadratic(p.a, int(mode)) == 0
    assert p.AddQuadraticConstraint(None, M, c) == 0
    return p, cost


def test_least_squares_beyond_lds_matches_the_oracle_and_lstsq():
    """x is numpy.linalg.lstsq's to ten times what the oracle's own answer achieves (X_VS_LSTSQ_ORACLE, asserted here to
    be what the oracle still achieves, within a factor of two); the oracle solves the program, and its t and the
    device's are lstsq's residual norm to the central path's gap."""
    A, b = least_squares_data()
    x_ls = np.linalg.lstsq(A, b, rcond=None)[0]
    t_ls = float(np.linalg.norm(A @ x_ls - b))
    p, cost = build_program()
    cfg = p.DefaultConfiguration()
    sol = p.Maximize(cost, cfg)
    M, c, _ = cone_data()
    o = ol.Program(UNKNOWNS + 1)
    assert o.add_quadratic(None, M, c) == 0
    oko, yo = o.solve(cost, copy_config(cfg))
    assert oko == 1 and sol.status == 1
    assert abs(yo[UNKNOWNS] - t_ls) <= T_VS_LSTSQ and abs(sol.y[UNKNOWNS] - t_ls) <= T_VS_LSTSQ
    measured = rel(yo[:UNKNOWNS], x_ls)
    print(f"oracle x against lstsq: {measured:.3g}; device x against lstsq: {rel(sol.y[:UNKNOWNS], x_ls):.3g}; "
          f"oracle t against lstsq: {abs(yo[UNKNOWNS] - t_ls):.3g}; device t: {abs(sol.y[UNKNOWNS] - t_ls):.3g}")
    assert 0.5 * X_VS_LSTSQ_ORACLE <= measured <= 2 * X_VS_LSTSQ_ORACLE, measured
    assert rel(sol.y[:UNKNOWNS], x_ls) <= 10 * X_VS_LSTSQ_ORACLE


def test_warm_started_resolve_of_a_streamed_quadratic_cone():
    """initialization_mode = 1 continues from the device's scaling points: get_W / set_W of a streamed cone."""
    p, cost = build_program()
    cfg = p.DefaultConfiguration()
    cold = p.Maximize(cost, cfg)
    assert cold.status == 1
    cfg.initialization_mode = 1
    warm = p.Maximize(cost, cfg)
    assert warm.status == 1


def test_with_the_switch_off_the_program_is_refused_as_before(capfd):
    p, cost = build_program(mode=0)
    sol = p.Maximize(cost, p.DefaultConfiguration())
    assert sol.status != 1
    assert "LDS" in capfd.readouterr().err
