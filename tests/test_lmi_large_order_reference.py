"""Matrix inequalities of any order, the parts a host decides: what cxk_finalize admits and refuses (host-only
contexts, device = -1), the switch and the counter, and the inputs of test_gpu_lmi_large_order.py checked by float64
alone: every short-run input breaks within a dozen steps and is determined by its data, and three quarters of the
long real recurrences are."""
import ctypes as C

import numpy as np
import pytest

import lmi_large_order_cases as lc
import lmi_reference as ref
from conex_amd import KktContext
from conex_amd.kkt import KktError


def identity_planes(d, n):
    E = np.zeros((d, n, n))
    E[0] = np.eye(n)
    return E


# ------------------------------------------------------------------------------------ admission
def test_order_1025_is_admitted():
    k = KktContext(1, device=-1)
    assert k.add_lmi(np.zeros((1, 1025, 1025)), np.eye(1025)) == 0
    k.initialize()
    assert k.count_wide_spectrum() == 0  # a host-only context chooses no kernels


@pytest.mark.parametrize("mode", [-1, 1])
def test_order_2550_is_admitted_with_the_chip_wide_run(mode):
    k = KktContext(1, device=-1)
    k.set_wide_spectrum(mode)
    assert k.add_lmi(np.zeros((1, 2550, 2550)), np.eye(2550)) == 0
    k.initialize()


MODE0 = (r"a matrix inequality whose \(real representation's\) order is above 2549 needs the chip-wide Lanczos run "
         r"\(cxk_set_wide_spectrum / CXK_WIDE_SPECTRUM, which is 0\)$")


def test_mode_0_refuses_orders_above_2549_by_name(monkeypatch):
    k = KktContext(1, device=-1)
    k.set_wide_spectrum(0)
    assert k.add_lmi(np.zeros((1, 2550, 2550)), np.eye(2550)) == 0
    with pytest.raises(KktError, match=MODE0):
        k.initialize()
    k = KktContext(1, device=-1)  # the real representation of a complex constraint of order 1275
    k.set_wide_spectrum(0)
    assert k.add_hermitian(np.zeros((1, 2, 1275, 1275)), identity_planes(2, 1275)) == 0
    with pytest.raises(KktError, match=MODE0):
        k.initialize()
    k = KktContext(1, device=-1)  # 2549 runs on one workgroup
    k.set_wide_spectrum(0)
    assert k.add_lmi(np.zeros((1, 2549, 2549)), np.eye(2549)) == 0
    k.initialize()
    monkeypatch.setenv("CXK_WIDE_SPECTRUM", "0")  # the environment's word where there is no call
    k = KktContext(1, device=-1)
    assert k.add_lmi(np.zeros((1, 2550, 2550)), np.eye(2550)) == 0
    with pytest.raises(KktError, match=MODE0):
        k.initialize()
    k = KktContext(1, device=-1)  # a call goes in front of it
    k.set_wide_spectrum(-1)
    assert k.add_lmi(np.zeros((1, 2550, 2550)), np.eye(2550)) == 0
    k.initialize()


def test_order_beyond_the_int_range_is_refused_by_name():
    """46341^2 > 2^31 - 1.  cxk_add_lmi copies nothing of such a constraint, so one double stands for its matrices."""
    k = KktContext(1, device=-1)
    one = np.zeros(1)
    ptr = one.ctypes.data_as(C.POINTER(C.c_double))
    assert k.L.cxk_add_lmi(k.h, 46341, 1, ptr, ptr, None) == 0
    with pytest.raises(KktError, match=r"a matrix inequality of order above 46340 is not supported "
                                       r"\(the kernels index its n x n entries with ints\)$"):
        k.initialize()


def test_the_factored_limits_stay():
    k = KktContext(1, device=-1)
    k.set_wide_spectrum(1)
    assert k.add_lmi_factored(np.ones((1025, 1)), [0, 1], None, np.eye(1025)) == 0
    with pytest.raises(KktError, match=r"a factored LMI of order above 1024 is not supported \(one panel row per thread in the Pade LU\)"):
        k.initialize()
    k = KktContext(1, device=-1)
    k.set_wide_spectrum(1)
    n = 1275  # N = 2550: one past LmiLargeSpectrumMaxOrder(), which keeps its value
    assert k.add_hermitian_factored(np.ones((2, n, 1)), [0, 1], None, identity_planes(2, n)) == 0
    with pytest.raises(KktError, match=r"order above 2549 .* 163328 B of LDS"):
        k.initialize()


def test_the_switch():
    k = KktContext(1, device=-1)
    assert k.count_wide_spectrum() == -1  # nothing is chosen before initialize
    for bad in (-2, 2):
        with pytest.raises(KktError, match=r"cxk_set_wide_spectrum.*mode"):
            k.set_wide_spectrum(bad)
    for ok in (-1, 0, 1):
        k.set_wide_spectrum(ok)
    assert k.add_lmi(np.zeros((1, 3, 3)), np.eye(3)) == 0
    k.initialize()
    with pytest.raises(KktError, match=r"cxk_set_wide_spectrum.*finalized"):
        k.set_wide_spectrum(1)
    assert k.count_wide_spectrum() == 0


def test_the_constants_are_the_kernel_matrix_tests():
    import test_gpu_lmi_kernel_matrix as km
    for name in ("C_PREPARE", "C_TAKE", "TOL_LANCZOS", "TOL_SPECTRUM", "STABLE", "C_WEIGHT"):
        assert getattr(lc, name) == getattr(km, name), name


# ------------------------------------------------------------------------------------ the GPU tests' data
@pytest.mark.parametrize("case", lc.SHORT_REAL + lc.SHORT_EDGE, ids=[c[0] for c in lc.SHORT_REAL + lc.SHORT_EDGE])
def test_short_real_inputs_break_within_a_dozen_steps_and_are_determined(case):
    _, n, m, shifts, seed = case
    A, Cm, y, exact = lc.short_run_lmi(n, m, shifts, seed)
    S = lc.minus_s(A, Cm, y)
    ev = np.linalg.eigvalsh(S)
    rho = max(abs(exact[0]), abs(exact[-1]))
    assert abs(ev[0] - exact[0]) <= 1e-12 * rho and abs(ev[-1] - exact[-1]) <= 1e-12 * rho
    W = np.eye(n)
    for r in lc.start_columns(S, S):  # W = I: WS = minus_s
        steps, lo, hi = lc.lanczos_count(S, W, r, n // 2)
        assert steps <= 12 and steps == len(exact), steps
        assert abs(lo - exact[0]) <= lc.TOL_LANCZOS * rho and abs(hi - exact[-1]) <= lc.TOL_LANCZOS * rho
        assert ref.ritz_spread(S, W, r, n // 2, trials=2) <= lc.STABLE * rho


def test_short_complex_input_has_three_eigenvalues():
    """Its minimal polynomial has degree three, so a Krylov space from any start vector has at most three dimensions
    (the Hermitian start vector and relative break are not restated here)."""
    _, n, m, shifts, seed = lc.SHORT_COMPLEX
    A, Cm, y, exact = lc.short_run_complex(n, m, shifts, seed)
    S = ref.complex_rep(lc.minus_s(A, Cm, y), 2)
    assert np.abs(S - S.conj().T).max() <= 1e-15
    ev = np.linalg.eigvalsh(S)
    assert np.all(np.min(np.abs(ev[:, None] - exact[None, :]), axis=1) <= 1e-12)
    assert abs(ev[0] - exact[0]) <= 1e-12 and abs(ev[-1] - exact[-1]) <= 1e-12


def test_three_quarters_of_the_long_real_runs_are_determined():
    flags = []
    for n, seed in lc.LONG_REAL:
        q, p, _ = lc.long_real_determined(n, seed)
        flags += [q, p]
    assert sum(flags) * 4 >= 3 * len(flags), flags


@pytest.mark.parametrize("case", lc.TALL_CASES, ids=lambda c: f"n{c[0]}")
def test_tall_panel_inputs_permute(case):
    """tall_case asserts that float64 partial pivoting swaps rows in the Pade system of its input."""
    lc.tall_case(*case)
