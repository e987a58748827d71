"""A max-cut relaxation given by its entries, end to end, and one assembly at an order whose dense form is never built.

Max-cut  max -sum y  s.t.  Diag(y) - Q >= 0  (Q = graph Laplacian / 4): A_i = -e_i e_i^T, C = -Q, b = -1
(synthetic.maxcut_entries is synthetic.maxcut_problem as lists, from the same random stream).
 - n = m = 70 through Conex.AddLinearMatrixInequalityFromEntries and through the dense entry point: the same status and
   iteration count, y to 1e-8, the dual's diagonal X_ii = -b_i (A_i^*(X) = -X_ii = b_i) to the 1e-5 that
   test_gpu_lmi_factored_solve.py asks of |b - A^* x|, and a warm-started re-solve.  At this order the automatic rule
   leaves the affine term on the two GEMMs (4 n^2 / (nnz C + positions) is about 20, below the measured constant), so the
   two programs run the same kernels on the same device lists.  (Asked for with SetSparseAffine(1), the new kernels end
   at the same point by another path: the interior-point iteration amplifies last-bit differences of the assembly,
   which is so between the two routes that were here before as well)
 - n = m = 1200 through KktContext.add_lmi_coo: expanded, the A_i are 13.8 GB, which are never allocated.  With a
   prescribed symmetric W the family has closed forms, G_ij = W_ij^2, AW_i = -W_ii, AQc_i = -(W C W)_ii,
   <c,Qc> = tr(C W C W), <w,c> = tr(C W), evaluated here by numpy; bars as in tests/test_gpu_sparse.py (Schur blocks
   1e-13, direction 1e-10).  No interior-point run at that order: its one-workgroup eigenvalue query takes hundreds of
   milliseconds a call.
"""
import numpy as np
import pytest

from conex_amd import KktContext
from conex_amd import synthetic as syn
from conex_amd.program import Conex
from test_gpu_parity import rel

pytestmark = pytest.mark.gpu


def from_entries(n):
    e = syn.maxcut_entries(n)
    p = Conex(n)
    assert p.AddLinearMatrixInequalityFromEntries(n, e["ptr"], e["row"], e["col"], e["val"]) == 0
    return p, e["b"]


def from_matrices(n):
    d = syn.maxcut_problem(n)
    p = Conex(n)
    p.AddDenseLinearMatrixInequality(np.transpose(d["A"][0], (1, 2, 0)), d["C"][0])
    return p, d["b"]


def iterations(p):
    return p.GetIterationNumberStats(-1).iteration_number + 1


def test_maxcut_by_entries_solves_as_the_dense_program_does():
    n = 70
    p, b = from_entries(n)
    q, _ = from_matrices(n)
    cfg = p.DefaultConfiguration()
    sol, ref = p.Maximize(b, cfg), q.Maximize(b, q.DefaultConfiguration())
    A = p._L
    print(f"status {sol.status} / {ref.status}, iterations {iterations(p)} / {iterations(q)}, "
          f"|y - y_dense| {np.max(np.abs(sol.y - ref.y)):.3g}, on the new kernels {A.CONEX_HIP_CountSparseAffine(p.a)} / "
          f"{A.CONEX_HIP_CountSparseAffine(q.a)}")
    assert A.CONEX_HIP_CountSparseAffine(q.a) == 0
    assert sol.status == ref.status == 1
    assert iterations(p) == iterations(q)
    assert np.allclose(sol.y, ref.y, rtol=1e-8, atol=1e-8)
    # Diag(y) - Q is positive semidefinite at the solution; the dual is feasible: X >= 0 with X_ii = -b_i = 1
    Q = syn.maxcut_problem(n)["Q"]
    assert np.linalg.eigvalsh(np.diag(sol.y) - Q).min() >= -1e-6
    X = p.GetDualVariables()[0]
    assert X.shape == (n, n) and np.linalg.eigvalsh(0.5 * (X + X.T)).min() >= -1e-9
    assert np.max(np.abs(np.diag(X) + b)) <= 1e-5, np.max(np.abs(np.diag(X) + b))
    _, err = p.ComputeErrors(sol.y, [X], b)  # (the operator and its adjoint from the entries)
    assert err.Ax_minus_b <= 1e-5 * np.sqrt(n) and err.min_eig_S[0] >= -1e-6
    # a warm-started re-solve converges to the same point
    cfg.initialization_mode = 1
    warm = p.Maximize(b, cfg)
    assert warm.status == 1
    assert np.allclose(warm.y, sol.y, rtol=1e-5, atol=1e-7)


def test_one_assembly_factor_and_solve_at_order_1200():
    n = 1200
    e = syn.maxcut_entries(n)
    k = KktContext(n, device=0)
    assert k.add_lmi_coo(n, e["ptr"], e["row"], e["col"], e["val"]) == 0
    k.initialize()
    assert k.count_sparse_lmi() == 1 and k.count_sparse_affine() == 1  # (the automatic rule: 4 n^2 against ~15 n)
    rng = np.random.default_rng(1200)
    S = rng.standard_normal((n, n))
    W = np.eye(n) + 0.3 * 0.5 * (S + S.T) / np.sqrt(n)  # symmetric, eigenvalues within 1 -+ 0.65
    k.set_W(0, W)
    k.assemble()
    G, AW, AQc, sc = k.constraint_schur(0)
    C_ = np.zeros((n, n))
    s = slice(e["ptr"][n], e["ptr"][n + 1])
    C_[e["row"][s], e["col"][s]] = e["val"][s]
    C_[e["col"][s], e["row"][s]] = e["val"][s]
    X = W @ C_ @ W
    print(f"G {rel(np.tril(G), np.tril(W * W)):.3g}, AW {rel(AW, -np.diag(W)):.3g}, AQc {rel(AQc, -np.diag(X)):.3g}, "
          f"<w,c> {abs(sc[0] - np.sum(C_ * W)) / abs(np.sum(C_ * W)):.3g}, "
          f"<c,Qc> {abs(sc[1] - np.sum(C_ * X)) / abs(np.sum(C_ * X)):.3g}")
    assert rel(np.tril(G), np.tril(W * W)) <= 1e-13
    assert rel(AW, -np.diag(W)) <= 1e-13 and rel(AQc, -np.diag(X)) <= 1e-13
    assert rel(sc, [np.sum(C_ * W), np.sum(C_ * X)]) <= 1e-13
    assert k.factor() == 1
    rhs = 0.7 * (e["b"] * 0.9 + AQc * 0.8) - 2 * AW
    y = k.solve_inplace(rhs)
    print(f"direction {rel(y, np.linalg.solve(W * W, rhs)):.3g}")
    assert rel(y, np.linalg.solve(W * W, rhs)) <= 1e-10
