"""The extended-precision LMI reference (lmi_reference.py) against the CPU oracle at well-conditioned
points: if the reference is wrong, this says so before any kernel comparison is read."""
import numpy as np
import pytest

import lmi_reference as ref
import oracle_lib as ol
from conex_amd import synthetic as syn

TOL = 1e-13


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    n = np.linalg.norm(b)
    return np.linalg.norm(a - b) / n if n > 0 else np.linalg.norm(a - b)


def one_constraint(kind, n, m, d, seed):
    """A K = 1 problem (A, C, W, y) of the given kind and the oracle program holding it."""
    rng = np.random.default_rng(seed)
    if kind == "herm":
        prob = syn.hermitian_problem(K=1, n=n, d=d, m=m, seed=seed)
        W = syn.hermitian_scaling_points(1, n, d, seed=seed + 1)[0]
    else:
        prob = syn.lmi_problem(K=1, n=n, m=m, seed=seed)
        if kind == "nonsym":
            prob["A"] = rng.uniform(-1, 1, prob["A"].shape)
        W = syn.scaling_points(1, n, seed=seed + 1)[0]
    o = syn.build(ol.Program, prob, "herm" if kind == "herm" else "lmi")
    o.set_W(0, W)
    y = rng.uniform(-0.1, 0.1, o.N)
    return prob["A"][0], prob["C"][0], W, y, o


CASES = [("sym", 6, 4, 0), ("sym", 20, 7, 0), ("nonsym", 7, 5, 0), ("herm", 5, 4, 2), ("herm", 4, 3, 4),
         ("herm", 5, 3, 1)]


@pytest.mark.parametrize("kind,n,m,d", CASES)
def test_schur_matches_the_oracle(kind, n, m, d):
    A, Cm, W, y, o = one_constraint(kind, n, m, d, seed=11 + n + d)
    r = ref.schur(A, Cm, W, d)
    o.assemble()
    Go, AWo, AQo, sco = o.constraint_schur(0)
    assert rel(np.tril(np.asarray(r["G"][0], dtype=np.float64)), np.tril(Go)) <= TOL
    assert rel(r["AW"][0], AWo) <= TOL and rel(r["AQc"][0], AQo) <= TOL and rel(r["sc"][0], sco) <= TOL
    for v, mag in r.values():  # a magnitude sum bounds its value
        assert np.all(np.abs(v) <= mag * (1 + 1e-15))


@pytest.mark.parametrize("kind,n,m,d", CASES)
def test_prepare_query_affine_and_take_match_the_oracle(kind, n, m, d):
    A, Cm, W, y, o = one_constraint(kind, n, m, d, seed=23 + n + d)
    c = 0.6
    p = ref.prepare(A, Cm, W, y, c, d)
    eo = o.weighted_slack_eigenvalues(y, c)
    assert rel(p["frob"][0], eo[2]) <= TOL and rel(p["trace"][0], eo[3]) <= TOL
    io = o.prepare_step(y, c, 1.0)
    assert rel(p["normsqrd"][0], io[0]) <= TOL
    if kind != "nonsym":  # Ritz values lie in the spectrum of W^1/2 (-S) W^1/2
        lo, hi = ref.slack_spectrum(A, Cm, W, y, c, d)
        rho = max(abs(lo), abs(hi))
        assert -hi - 1e-12 * rho <= eo[0] <= eo[1] <= -lo + 1e-12 * rho
        assert io[1] <= max(abs(1 + lo), abs(1 + hi)) + 1e-12 * rho
    step = min(1.0, 2.0 / io[1] ** 2)
    Wn, Wm, growth = ref.take_step(A, Cm, W, y, c, 1.0, step, d)
    o.take_step(step)
    assert rel(Wn, o.get_W(0)) <= TOL
    assert growth >= 1.0
    # the affine update from the same point
    o.set_W(0, W)
    Wa, _ = ref.affine(A, Cm, W, y, c, 0.3, d)
    o.prepare_step(y, c, 0.3, affine=1)
    assert rel(Wa.T if d == 0 else Wa, o.get_W(0)) <= TOL  # (an LMI's W comes back column-major)


@pytest.mark.parametrize("d", [2, 4])
def test_complex_representation_is_multiplicative(d):
    rng = np.random.default_rng(d)
    X, Y = rng.uniform(-1, 1, (2, d, 5, 5))
    Z = np.asarray(ref.hc_mul(ref.ld(X), ref.ld(Y)), dtype=np.float64)
    assert np.allclose(ref.complex_rep(Z, d), ref.complex_rep(X, d) @ ref.complex_rep(Y, d), atol=1e-13)


@pytest.mark.parametrize("cond", [1e6, 1e10])
def test_ill_conditioned_scaling_points(cond):
    rng = np.random.default_rng(5)
    W = ref.ill_conditioned_W(rng, 12, cond)
    lam = np.linalg.eigvalsh(W)
    assert lam[0] > 0 and abs(np.log10(lam[-1] / lam[0]) - np.log10(cond)) < 0.05
    for d in (2, 4):
        Wh = ref.ill_conditioned_hermitian_W(rng, 6, d, cond)
        assert Wh.shape == (d, 6, 6)
        lam = np.linalg.eigvalsh(ref.complex_rep(Wh, d))
        assert lam[0] > 0 and abs(np.log10(lam[-1] / lam[0]) - np.log10(cond)) < 0.05
        assert np.allclose(Wh[0], Wh[0].T) and all(np.allclose(Wh[p], -Wh[p].T) for p in range(1, d))


def test_lu_solve():
    rng = np.random.default_rng(3)
    M = ref.ld(rng.uniform(-1, 1, (9, 9)))
    B = ref.ld(rng.uniform(-1, 1, (9, 4)))
    X = ref.lu_solve(M, B)
    assert float(np.max(np.abs(M @ X - B))) <= 1e-16
