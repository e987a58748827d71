"""One interior-point solve through conex.h at an order past the old panel of the Pade LU: a dense LMI of order 1040
under CXK_WIDE_SPECTRUM=1 (the chip-wide Lanczos run; the one-workgroup run would take a minute)."""
import numpy as np
import pytest

import lmi_large_order_cases as lc

pytestmark = pytest.mark.gpu

# opt - b'y of the same construction and configuration at order 1024, the largest order the one-workgroup kernels run,
# measured on the commit before these orders were admitted (automatic mode gives the same bits on this one)
GAP_AT_1024 = 2.0021134949921304e-06  # measured on an MI355X


def test_dense_lmi_of_order_1040_solves_through_conex_h(monkeypatch):
    """max y_1 + y_2  s.t.  Q diag(C_1 - y_1 I, C_2 - y_2 I) Q' >= 0; the optimum is lambda_min(C_1) + lambda_min(C_2).
    The gap may be twice what order 1024 leaves (GAP_AT_1024, measured: 2.0021e-06; order 1040 measured 2.0019e-06): it
    scales with the order, which moves by 1.6 %; the rest is for the Lanczos estimates' sensitivity to summation
    order."""
    monkeypatch.setenv("CXK_WIDE_SPECTRUM", "1")
    monkeypatch.delenv("CXK_SPARSE_LMI", raising=False)
    A, Cm, b, opt = lc.solve_case(1040)
    ok, y = lc.solve_dense_lmi(A, Cm, b)
    assert ok == 1
    gap = opt - b @ y
    lam = np.linalg.eigvalsh(Cm - np.tensordot(y, A, axes=1))[0]
    print(f"order 1040: opt - b'y = {gap:.6g}, lambda_min of the slack {lam:.3g}")
    assert lam >= -1e-6 * np.linalg.norm(Cm, 2)
    assert 0 <= gap <= 2 * GAP_AT_1024
