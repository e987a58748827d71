"""A complex Hermitian program of the line family (synthetic.hermitian_entries: every A_i one bus and one line, C = I),
order 12 over 12 variables, end to end: given once by its entries (Conex.AddHermitianMatrixInequalityFromEntries) and
once entry by entry through the dense Hermitian builders (NewLinearMatrixInequality / UpdateLinearOperator /
UpdateAffineTerm, which end in cxk_add_hermitian).  The same status and iteration count, and the objective and y within
the bars tests/test_gpu_lmi_entries_solve.py asks of its pair (1e-8).

 - test_..._as_the_dense_hermitian_program_does: each program on its own route, the entries on the folded sparse
   kernels, the dense planes of order 24 real on lmi_schur_mfma.  This is the test of lmi_fold_project: inside a run W
   is what TakeStep left, a real representation only up to rounding, and folded sums over W as stored read one block
   row of that deviation where the unfolded ones average it.  Measured on an MI355X without the projection:
   14 iterations against 13 and |y - y_dense| = 3.3e-5 (five other seeds: 1e-6 to 1.6e-4); with it 13 / 13 and
   2.6e-10 (the others 1.5e-11 to 5.8e-9), as the unfolded sparse kernels give against the same reference (2.1e-10).
 - test_..._on_the_same_kernels: CXK_SPARSE_LMI=1 and CXK_SPARSE_FOLD=1 send the program built from dense planes to the
   folded sparse kernels too, on the lists read off its real representations: a whole interior-point run on the lists
   that cxk_add_hermitian_coo builds directly against those lists."""
import numpy as np
import pytest

from conex_amd import synthetic as syn
from conex_amd.program import Conex

pytestmark = pytest.mark.gpu


def iterations(p):
    return p.GetIterationNumberStats(-1).iteration_number + 1


def solve_pair(folded_reference):
    n = m = 12
    e = syn.hermitian_entries(n, 2, m)
    p = Conex(m)
    assert p.AddHermitianMatrixInequalityFromEntries(n, 2, e["ptr"], e["row"], e["col"], e["val"]) == 0
    q = Conex(m)
    cid = q.NewLinearMatrixInequality(n, 2)
    for i in range(m + 1):
        for s in range(e["ptr"][i], e["ptr"][i + 1]):
            for plane in range(2):
                v = float(e["val"][s, plane])
                if v == 0.0:
                    continue
                if i < m:
                    q.UpdateLinearOperator(cid, v, i, int(e["row"][s]), int(e["col"][s]), plane)
                else:
                    q.UpdateAffineTerm(cid, v, int(e["row"][s]), int(e["col"][s]), plane)
    sol, ref = p.Maximize(e["b"], p.DefaultConfiguration()), q.Maximize(e["b"], q.DefaultConfiguration())
    A = p._L
    print(f"status {sol.status} / {ref.status}, iterations {iterations(p)} / {iterations(q)}, "
          f"|y - y_dense| {np.max(np.abs(sol.y - ref.y)):.3g}, objective {e['b'] @ sol.y:.12g} / {e['b'] @ ref.y:.12g}, "
          f"folded {A.CONEX_HIP_CountSparseFold(p.a)} / {A.CONEX_HIP_CountSparseFold(q.a)}")
    assert A.CONEX_HIP_CountSparseFold(p.a) == 1 and A.CONEX_HIP_CountSparseFold(q.a) == folded_reference
    assert sol.status == ref.status == 1
    assert iterations(p) == iterations(q)
    assert np.allclose(sol.y, ref.y, rtol=1e-8, atol=1e-8)
    assert np.isclose(e["b"] @ sol.y, e["b"] @ ref.y, rtol=1e-8, atol=1e-8)
    # C - sum y_i A_i is positive semidefinite at the solution (the planes of the same data)
    S = e["C"] - np.einsum("i,idjk->djk", sol.y, e["A"])
    assert np.linalg.eigvalsh(S[0] + 1j * S[1]).min() >= -1e-6
    X = p.GetDualVariables()[0]                                            # (the real plane)
    assert X.shape == (n, n)


def test_the_line_family_by_entries_solves_as_the_dense_hermitian_program_does():
    solve_pair(0)


def test_the_line_family_by_entries_solves_as_the_dense_hermitian_program_does_on_the_same_kernels(monkeypatch):
    monkeypatch.setenv("CXK_SPARSE_LMI", "1")
    monkeypatch.setenv("CXK_SPARSE_FOLD", "1")
    solve_pair(1)
