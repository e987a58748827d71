"""Matrix inequalities beyond the one-workgroup limits of the large-order route: the take step past the 1024-row
panel of the Pade LU (lu_panel_tall), the chip-wide Lanczos run (kernels_lmi_wide.hip.h) against the one-workgroup
run on long recurrences, orders past the LDS ceiling of 2549 on short recurrences with known eigenvalues, and a
context that mixes old and new.  Inputs and float64 restatements: lmi_large_order_cases.py (checked by float64 alone
in test_lmi_large_order_reference.py).  Bounds: the constants of test_gpu_lmi_kernel_matrix.py; the take step's is
twice that file's, because the reference here is float64 too."""
import numpy as np
import pytest

import lmi_large_order_cases as lc
import lmi_reference as ref
from conex_amd import KktContext

pytestmark = pytest.mark.gpu

U = lc.U
SWITCHES = ("CXK_SPARSE_LMI", "CXK_WIDE_SPECTRUM", "CXK_WIDE_REDUCE_MIN_ORDER", "CXK_LMI_SCHUR", "CXK_GEMM_MIN_N", "CXK_GRAM_SPLITS", "CXK_NO_HERM_FOLD")


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)


def context(kind, A, Cm, mode):
    """One constraint over all of its variables; mode None: no call (automatic)."""
    k = KktContext(A.shape[0], device=0)
    if mode is not None:
        k.set_wide_spectrum(mode)
    assert (k.add_hermitian if kind == "herm" else k.add_lmi)(A, Cm) == 0
    k.initialize()
    return k


def within(gpu, val, mag, c, what):
    err = np.abs(np.asarray(gpu, dtype=np.float64) - np.asarray(val, dtype=np.float64))
    bound = c * U * np.asarray(mag, dtype=np.float64)
    worst = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
    print(f"{what}: error {worst:.3g} x the bound c u |.| (c = {c:.3g})")
    assert np.all(err <= bound), f"{what}: error {worst:.3g} x the bound c u |.| (c = {c:.3g})"


def check_take_step(k, A, Cm, W, y, e_weight, step, d, what):
    Wn, Wm, growth = lc.take_step64(A, Cm, W, y, lc.C_WEIGHT, e_weight, step, d)
    got = k.get_W(0).reshape(np.shape(Wn))
    if d == 0:
        Wn, Wm = Wn.T, Wm.T
    within(got, Wn, Wm, 2 * lc.C_TAKE * growth, f"{what}: W after the step (growth {growth:.3g})")


# ------------------------------------------------------------------ a. TakeStep past the old panel
@pytest.mark.parametrize("case", lc.TALL_CASES, ids=lambda c: f"n{c[0]}" + ("-sparse" if c[2] else ""))
def test_take_step_past_the_old_panel(case, monkeypatch):
    n, seed, sparse = case
    if sparse:
        monkeypatch.setenv("CXK_SPARSE_LMI", "1")
    A, Cm, y, W = lc.tall_case(n, seed, sparse)
    k = context("lmi", A, Cm, 1)
    assert k.count_wide_spectrum() == 1 and k.count_sparse_lmi() == (1 if sparse else 0)
    assert k.lmi_kernels(0)["take"] == "LmiLargeTakeStep pade" and k.lmi_kernels(0)["prepare"] == "LmiLargePrepare<0>"
    k.set_W(0, W)
    k.prepare_step(y, lc.C_WEIGHT, lc.E_WEIGHT)
    k.take_step(lc.STEP, lc.E_WEIGHT)
    check_take_step(k, A, Cm, W, y, lc.E_WEIGHT, lc.STEP, 0, f"order {n}")


# ------------------------------------------------------------------ b. chip-wide against one workgroup, long runs
def agree(a, b, mag, what):
    bound = lc.C_PREPARE * U * float(mag)
    print(f"{what}: |{a!r} - {b!r}| = {abs(a - b):.3g}, bound {bound:.3g}")
    assert abs(a - b) <= bound, what


def run_three(kind, A, Cm, W, y):
    """(query, PrepareStep info) under mode 0, mode 1 and mode 1 again (fresh contexts: the same call numbers)."""
    runs = []
    for mode in (0, 1, 1):
        k = context(kind, A, Cm, mode)
        assert k.count_wide_spectrum() == mode
        assert k.lmi_kernels(0)["prepare"] == "LmiLargePrepare<0>" and k.lmi_kernels(0)["query"] == "LmiLargePrepare<1>"
        k.set_W(0, W)
        ek = k.weighted_slack_eigenvalues(y, lc.C_WEIGHT)
        info = k.prepare_step(y, lc.C_WEIGHT, 1.0)
        runs.append((ek, info))
        k.close()
    return runs


def compare_modes(runs, p, spec, det_q, det_p):
    (e0, i0), (e1, i1), (e2, i2) = runs
    assert e1.tobytes() == e2.tobytes() and i1.tobytes() == i2.tobytes(), "two chip-wide runs differ in their bits"
    agree(e1[2], e0[2], p["frob"][1], "frob")
    agree(e1[3], e0[3], p["trace"][1], "trace")
    agree(i1[0], i0[0], p["normsqrd"][1], "normsqrd")
    lo, hi = spec
    rho = max(abs(lo), abs(hi))
    tol = lc.TOL_SPECTRUM * rho
    assert -hi - tol <= e1[0] <= e1[1] <= -lo + tol, (e1, spec)
    assert i1[1] <= max(abs(1 + lo), abs(1 + hi)) + tol, (i1, spec)
    if det_q:
        assert abs(e1[0] - e0[0]) <= lc.TOL_LANCZOS * rho and abs(e1[1] - e0[1]) <= lc.TOL_LANCZOS * rho, (e0, e1)
    if det_p:
        assert abs(i1[1] - i0[1]) <= lc.TOL_LANCZOS * rho, (i0, i1)


def pick_reduce(monkeypatch, reduce):
    """The partials of a pass summed by lmi_wide_reduce (from order 2049 on by itself) or by lmi_wide_step."""
    if reduce:
        monkeypatch.setenv("CXK_WIDE_REDUCE_MIN_ORDER", "0")


REDUCE = pytest.mark.parametrize("reduce", [False, True], ids=["step-sums", "reduce-launch"])


@REDUCE
@pytest.mark.parametrize("n,seed", lc.LONG_REAL, ids=[f"n{c[0]}" for c in lc.LONG_REAL])
def test_chip_wide_run_against_one_workgroup_real(n, seed, reduce, monkeypatch):
    pick_reduce(monkeypatch, reduce)
    prob, W, y = lc.long_real_case(n, seed)
    A, Cm = prob["A"][0], prob["C"][0]
    det_q, det_p, spec = lc.long_real_determined(n, seed)
    p = ref.prepare(A, Cm, W[0], y, lc.C_WEIGHT, 0)
    compare_modes(run_three("lmi", A, Cm, W[0], y), p, spec, det_q, det_p)


@REDUCE
@pytest.mark.parametrize("n,seed", lc.LONG_COMPLEX, ids=[f"c{c[0]}" for c in lc.LONG_COMPLEX])
def test_chip_wide_run_against_one_workgroup_complex(n, seed, reduce, monkeypatch):
    pick_reduce(monkeypatch, reduce)
    prob, W, y = lc.long_complex_case(n, seed)
    A, Cm = prob["A"][0], prob["C"][0]
    spec = ref.slack_spectrum(A, Cm, W[0], y, lc.C_WEIGHT, 2)
    p = ref.prepare(A, Cm, W[0], y, lc.C_WEIGHT, 2)
    # (Hermitian data at a well-conditioned point: determined, as in test_gpu_lmi_kernel_matrix.py)
    compare_modes(run_three("herm", A, Cm, W[0], y), p, spec, True, True)


# ------------------------------------------------------------------ c. past the LDS ceiling, short runs
E_SHORT = 3.0  # X = (WS + 3 I) step: eigenvalues on both sides of the Pade denominator's root for step 2


def check_short(k, A, Cm, y, exact, d, step, what):
    n = A.shape[-1]
    W = np.eye(n) if d == 0 else np.stack([np.eye(n)] + [np.zeros((n, n))] * (d - 1))
    lo, hi = exact[0], exact[-1]
    rho = max(abs(lo), abs(hi))
    p = lc.prepare64(A, Cm, W, y, lc.C_WEIGHT, d)
    ek = k.weighted_slack_eigenvalues(y, lc.C_WEIGHT)  # W = I: WS = minus_s; (-max, -min, frob, trace)
    print(what, "query", ek, "exact", -hi, -lo)
    assert abs(ek[0] + hi) <= lc.TOL_LANCZOS * rho and abs(ek[1] + lo) <= lc.TOL_LANCZOS * rho, (ek, exact)
    within(ek[2], *p["frob"], lc.C_PREPARE, f"{what}: frob")
    within(ek[3], *p["trace"], lc.C_PREPARE, f"{what}: trace")
    info = k.prepare_step(y, lc.C_WEIGHT, E_SHORT)
    print(what, "prepare", info)
    within(info[0], *p["normsqrd"], lc.C_PREPARE, f"{what}: normsqrd")
    assert abs(info[1] - max(abs(E_SHORT + lo), abs(E_SHORT + hi))) <= lc.TOL_LANCZOS * rho, (info, exact)
    k.take_step(step, E_SHORT)
    check_take_step(k, A, Cm, W, y, E_SHORT, step, d, what)


@pytest.mark.parametrize("case", lc.SHORT_REAL, ids=[c[0] for c in lc.SHORT_REAL])
def test_real_order_2550(case):
    cid, n, m, shifts, seed = case
    A, Cm, y, exact = lc.short_run_lmi(n, m, shifts, seed)
    k = context("lmi", A, Cm, None)
    assert k.count_wide_spectrum() == 1
    check_short(k, A, Cm, y, exact, 0, 2.0, f"order {n} {cid}")


@pytest.mark.parametrize("case", lc.SHORT_EDGE, ids=[c[0] for c in lc.SHORT_EDGE])
def test_real_orders_at_the_edge_of_the_reduce_launch(case):
    cid, n, m, shifts, seed = case
    A, Cm, y, exact = lc.short_run_lmi(n, m, shifts, seed)
    k = context("lmi", A, Cm, 1)
    assert k.count_wide_spectrum() == 1
    check_short(k, A, Cm, y, exact, 0, 2.0, f"order {n} {cid}")


def test_complex_order_1275_under_automatic_mode():
    cid, n, m, shifts, seed = lc.SHORT_COMPLEX
    A, Cm, y, exact = lc.short_run_complex(n, m, shifts, seed)
    k = context("herm", A, Cm, None)
    assert k.count_wide_spectrum() == 1
    assert k.lmi_kernels(0)["take"] == "LmiLargeTakeStep taylor"
    check_short(k, A, Cm, y, exact, 2, 0.5, f"complex order {n}")


# ------------------------------------------------------------------ d. a context mixing old and new
def test_mixed_context_keeps_the_existing_route_bit_for_bit():
    _, n, m, shifts, seed = lc.SHORT_REAL[0]
    Ab, Cb, yb, _ = lc.short_run_lmi(n, m, shifts, seed)
    prob, W70, y70 = lc.long_real_case(70, 9)
    A70, C70 = prob["A"][0], prob["C"][0]
    rng = np.random.default_rng(10)
    Al, cl, yl = rng.uniform(-1, 1, (5, 2)), np.ones(5), np.array([0.1, -0.2])

    def run(with_big):
        off = m if with_big else 0
        k = KktContext(off + 6, device=0)
        if with_big:
            assert k.add_lmi(Ab, Cb, list(range(m))) == 0
        i70 = k.add_lmi(A70, C70, list(range(off, off + 4)))
        assert k.add_linear(Al, cl, [off + 4, off + 5]) == i70 + 1
        k.initialize()
        assert k.count_wide_spectrum() == (1 if with_big else 0)
        k.set_W(i70, W70[0])
        y = np.concatenate(([yb] if with_big else []) + [y70, yl])
        k.assemble()
        out = [np.concatenate([np.ravel(x) for x in k.constraint_schur(i70)])]
        k.prepare_step(y, lc.C_WEIGHT, 1.0)
        out.append(k.step_info()[i70].copy())
        k.take_step(0.5, 1.0)
        out.append(k.get_W(i70).copy())
        return out

    for a, b in zip(run(True), run(False)):
        assert a.tobytes() == b.tobytes()
