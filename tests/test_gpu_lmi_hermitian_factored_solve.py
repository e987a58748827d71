"""Programs whose Hermitian matrix inequality is given by factors, end to end through
Conex.AddFactoredHermitianMatrixInequality, against the same program entered entry by entry through
NewLinearMatrixInequality(order, d) / UpdateLinearOperator / UpdateAffineTerm (the expanded planes).

PhaseLift shape: n = 6 complex, m = 12 rank-one measurements a_i a_i^*; maximize b'y subject to
C - sum_i y_i a_i a_i^* >= 0.  One quaternion case at n = 3, m = 8.

The two forms are compared in y, so y must be determined by the program.  C and b are therefore built from a strictly
complementary optimal pair: X* = f(H) of rank r and S* = g(H) of rank n - r for one random Hermitian H (functions of H
commute, X* S* = 0), y* random, C = S* + sum y*_i A_i, b_i = <A_i, X*>.  The pair is nondegenerate, y and X both
unique, when  dim Herm(r) <= m <= dim Herm(n) - dim Herm(n - r)  (Alizadeh, Haeberly, Overton 1997, over C and H with
dim Herm(k) = k^2 and k (2k - 1)): n = 6 complex, r = 3: 9 <= 12 <= 27; n = 3 quaternion, r = 2: 6 <= 8 <= 14.
(With C and b from a full-rank X0 the optimal X of such a program has rank 1 or 2, G = tr(A_i X A_j X) is singular at
the optimum for m = 12 > r^2, and y is determined to no more than the solve's own tolerance.)

Both forms must report the same status and iteration count; y and the dual's real plane agree to rtol 1e-6,
atol 1e-8, the tolerances of test_gpu_lmi_factored_solve.py.

Measured on the MI355X: status 1 / 1, 16 / 16 and 15 / 15 iterations, max |y - y_entry| = 1.1e-10 and 1.5e-11,
max |X - X_entry| = 8e-12 and 6e-12; y is 7e-7 and 4e-7 from y* in both forms (the dual's real plane 2e-5 from X*'s in
both forms at the default options: printed, not asserted).  Before the assembly projected W onto the real
representations (lmi_factored_herm_project) the two forms' y were 1e-5 apart at equal iteration counts.
"""
import numpy as np
import pytest

import lmi_reference as ref
from conex_amd import synthetic as syn
from conex_amd.program import Conex

pytestmark = pytest.mark.gpu


def planes_of(E, d, n):
    """The d planes of a matrix in the image of lmi_reference.complex_rep."""
    if d == 2:
        return np.stack([E.real, E.imag])
    a, b = E[:n, :n], E[:n, n:]
    return np.stack([a.real, a.imag, b.real, -b.imag])


def complementary_program(n, d, m, r, seed):
    """Rank-one factors a_i, C and b with the optimal pair (y*, X*) of the module's docstring."""
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((d, n, m))
    ptr, sg = np.arange(m + 1), np.ones(m)
    A = syn.expand_hermitian_factors(F, ptr, sg)
    lam, Q = np.linalg.eigh(ref.complex_rep(syn.random_hermitian(rng, d, n), d))
    mult = d // 2  # (every eigenvalue of a quaternion matrix appears twice in the complex representation)
    pair = np.arange(len(lam)) // mult  # eigh sorts ascending: the n eigenvalues, smallest first
    top = pair >= n - r
    wx, ws = rng.uniform(0.5, 1.5, n)[pair], rng.uniform(0.5, 1.5, n)[pair]  # (functions of H: one weight per eigenvalue)
    X = planes_of((Q * np.where(top, wx, 0.0)) @ Q.conj().T, d, n)
    S = planes_of((Q * np.where(top, 0.0, ws)) @ Q.conj().T, d, n)
    for P in (X, S):
        P[0] = 0.5 * (P[0] + P[0].T)
        P[1:] = 0.5 * (P[1:] - np.swapaxes(P[1:], -1, -2))
    assert np.abs(syn.hc_multiply(X, S)).max() <= 1e-12
    y = rng.uniform(-0.5, 0.5, m)
    C = S + np.tensordot(y, A, axes=1)
    b = np.einsum("ipab,pab->i", A, X)
    return dict(F=F, rank_ptr=ptr, sigma=sg, A=A, C=C, b=b, n=n, d=d, m=m, y=y, X=X)


def build_both(prob):
    n, d, m = prob["n"], prob["d"], prob["m"]
    A, Cm = prob["A"], prob["C"]
    f = Conex(m)
    assert f.AddFactoredHermitianMatrixInequality(prob["F"], prob["rank_ptr"], prob["sigma"], Cm) == 0
    e = Conex(m)
    cid = e.NewLinearMatrixInequality(n, d)
    for p in range(d):
        for col in range(n):
            for row in range(col if p == 0 else col + 1, n):
                for i in range(m):
                    e.UpdateLinearOperator(cid, A[i, p, row, col], i, row, col, p)
                e.UpdateAffineTerm(cid, Cm[p, row, col], row, col, p)
    return f, e


def solve_both(prob):
    f, e = build_both(prob)
    out = []
    for p in (f, e):
        sol = p.Maximize(prob["b"], p.DefaultConfiguration())
        out.append((sol, p.GetIterationNumberStats(-1).iteration_number + 1, p.GetDualVariables()[0]))
    (sf, itf, Xf), (se, ite, Xe) = out
    print(f"status {sf.status} / {se.status}, iterations {itf} / {ite}, |y - ye| {np.max(np.abs(sf.y - se.y)):.3g}, "
          f"|X - Xe| {np.max(np.abs(Xf - Xe)):.3g}, |y - y*| {np.max(np.abs(sf.y - prob['y'])):.3g}, "
          f"|X - X*| {np.max(np.abs(Xf - prob['X'][0])):.3g}")
    assert sf.status == se.status == 1
    assert itf == ite
    assert np.allclose(sf.y, se.y, rtol=1e-6, atol=1e-8)
    assert np.allclose(Xf, Xe, rtol=1e-6, atol=1e-8)
    n = prob["n"]
    assert Xf.shape == (n, n) and np.allclose(Xf, Xf.T, atol=1e-9 * np.abs(Xf).max())
    # the optimum the program was built from (1e-5: what test_python_frontend.py asks after a solve at the default options)
    assert np.allclose(sf.y, prob["y"], rtol=0, atol=1e-5 * max(1.0, np.abs(prob["y"]).max()))


def test_complex_phaselift_shape_matches_the_expanded_entry():
    solve_both(complementary_program(n=6, d=2, m=12, r=3, seed=2041))


def test_quaternion_rank_one_program_matches_the_expanded_entry():
    solve_both(complementary_program(n=3, d=4, m=8, r=2, seed=2042))
