"""Every kernel instance of the three per-constraint LMI stages (Schur assembly, PrepareStep with the
eigenvalue query and the affine update, TakeStep), at its dispatch edges, against the
extended-precision reference of lmi_reference.py.

Each row of CASES is a problem, the switches it runs under and the instance every stage must
dispatch (KktContext.lmi_kernels).  Each row runs at three scaling points: the suite's usual
well-conditioned ones and W of condition 1e6 and 1e10.  Results are compared entry by entry,
|gpu - ref| <= c u * (magnitude sum), with one constant c per quantity below; the take step's bound
also carries the reference's growth factor (cond(V - U) of the Pade solve, 1 for the Taylor form).
The Lanczos outputs have no exact reference: they are compared with the oracle as check_newton_step
does (lmax, the converged end, always), and must lie in the true spectral interval wherever the
reference's run is determined by its input (lanczos_determined), where lmin and the step's norminfd
are compared with the oracle as well.  The last test checks that the rows name every
instance the library can report.
"""
import numpy as np
import pytest

import lmi_reference as ref
import oracle_lib as ol
from conex_amd import KktContext, lmi_kernel_names
from conex_amd import synthetic as syn

pytestmark = pytest.mark.gpu

U = ref.U64
C_SCHUR = 64      # G, AW, AQc, <C, W>, <C, W C W>
C_PREPARE = 64    # normsqrd, the query's frob and trace
C_AFFINE = 32     # W (1 + e) + WS W
C_TAKE = 256      # sym(E W): E from the device's own WS, times the reference's growth factor
TOL_LANCZOS = 1e-6  # Ritz values against the oracle's, relative to the spectral radius
TOL_SPECTRUM = 1e-12  # Ritz values outside the true spectral interval, relative to its radius
STABLE = 1e-9       # a Lanczos run is determined by its input when last-bit changes move it less than this
POINTS = ("well", 1e6, 1e10)
C_WEIGHT = 1.0    # minus_s = sum y_i A_i - C = -S


def names(schur, prep, take, n, large=False):
    """Expected {stage: name}; prep in rows-packed / rows-unpacked / odd / even / g20 / g0 / large."""
    p = {"rows-packed": "lmi_prepare_rows<{},20,exact> packed", "rows-unpacked": "lmi_prepare_rows<{},20,exact> unpacked",
         "odd": "lmi_prepare_rows<{},20> odd", "even": "lmi_prepare_rows<{},20> even",
         "g20": "lmi_prepare_generic<{},20>", "g0": "lmi_prepare_generic<{},0>", "large": "LmiLargePrepare<{}>"}[prep]
    affine = ("LmiLargePrepare<0> affine" if prep == "large" else
              "lmi_prepare_generic<0,20> affine" if n == 20 else "lmi_prepare_generic<0,0> affine")
    return dict(schur=schur, prepare=p.format(0), query=p.format(1), take=take, affine=affine)


MF = "lmi_schur_mfma<{}> {} {}"
R20P, R20E = "lmi_take_step_rows<20> padded", "lmi_take_step_rows<20> exact"
R32P, R32E = "lmi_take_step_rows<32> padded", "lmi_take_step_rows<32> exact"
T24P, T24E = "lmi_take_step_rows_taylor<24> padded", "lmi_take_step_rows_taylor<24> exact"
T32P, T32E = "lmi_take_step_rows_taylor<32> padded", "lmi_take_step_rows_taylor<32> exact"
GEMM = "schur_gemm {} {}{}"
ONE = {"CXK_GRAM_SPLITS": "1"}

# (id, kind, K, n, m, d, env, expected); kind: sym / nonsym / herm / sparse / sparse-densec
CASES = [
    # the literal kernels (non-symmetric data)
    ("literal-7", "nonsym", 3, 7, 5, 0, {}, names("lmi_schur_generic literal", "g0", "lmi_take_step_generic<0>", 7)),
    ("literal-20", "nonsym", 2, 20, 6, 0, {}, names("lmi_schur_generic literal", "g20", "lmi_take_step_generic<20>", 20)),
    # the symmetric LDS kernel: by request, and below gemm_min_n = 9 without an MFMA instance
    ("generic-forced", "sym", 3, 7, 5, 0, {"CXK_LMI_SCHUR": "generic"}, names("lmi_schur_generic symmetric", "odd", R20P, 7)),
    ("generic-n8-m32", "sym", 2, 8, 32, 0, {}, names("lmi_schur_generic symmetric", "even", R20P, 8)),
    ("gemm-n9-m32", "sym", 2, 9, 32, 0, {}, names(GEMM.format("full", "lds", ""), "odd", R20P, 9)),
    # lmi_schur_mfma, every instance exact / padded, two / one P image, and the tile limits
    ("mfma8", "sym", 3, 8, 5, 0, {}, names(MF.format(8, "exact", "two-images"), "even", R20P, 8)),
    ("mfma8-pad-n3", "sym", 3, 3, 2, 0, {}, names(MF.format(8, "padded", "two-images"), "odd", R20P, 3)),
    ("mfma8-pad-n2", "sym", 2, 2, 2, 0, {}, names(MF.format(8, "padded", "two-images"), "g0", R20P, 2)),
    ("mfma12", "sym", 3, 12, 9, 0, {}, names(MF.format(12, "exact", "two-images"), "even", R20P, 12)),
    ("mfma12-pad-m31", "sym", 2, 11, 31, 0, {}, names(MF.format(12, "padded", "two-images"), "odd", R20P, 11)),
    ("n12-m32", "sym", 3, 12, 32, 0, {}, names(GEMM.format("full", "lds", " split"), "even", R20P, 12)),
    ("mfma16", "sym", 3, 16, 16, 0, {}, names(MF.format(16, "exact", "two-images"), "even", R20P, 16)),
    ("mfma16-single", "sym", 2, 16, 30, 0, {}, names(MF.format(16, "exact", "one-image"), "even", R20P, 16)),
    ("mfma16-pad", "sym", 3, 13, 10, 0, {}, names(MF.format(16, "padded", "two-images"), "odd", R20P, 13)),
    ("mfma16-pad-single", "sym", 2, 14, 31, 0, {}, names(MF.format(16, "padded", "one-image"), "even", R20P, 14)),
    ("mfma20", "sym", 3, 20, 20, 0, {}, names(MF.format(20, "exact", "two-images"), "rows-packed", R20E, 20)),
    ("mfma20-many", "sym", 300, 20, 20, 0, {}, names(MF.format(20, "exact", "two-images"), "rows-packed", R20E, 20)),
    ("mfma20-single-m23", "sym", 2, 20, 23, 0, {}, names(MF.format(20, "exact", "one-image"), "rows-packed", R20E, 20)),
    ("n20-m24", "sym", 2, 20, 24, 0, {}, names(GEMM.format("full", "lds", " split"), "rows-packed", R20E, 20)),
    ("mfma20-pad", "sym", 3, 18, 9, 0, {}, names(MF.format(20, "padded", "two-images"), "even", R20P, 18)),
    ("mfma20-pad-single", "sym", 2, 19, 22, 0, {}, names(MF.format(20, "padded", "one-image"), "odd", R20P, 19)),
    ("mfma24", "sym", 3, 24, 10, 0, {}, names(MF.format(24, "exact", "two-images"), "g0", R32P, 24)),
    ("mfma24-single-m20", "sym", 2, 24, 20, 0, {}, names(MF.format(24, "exact", "one-image"), "g0", R32P, 24)),
    ("n24-m21", "sym", 2, 24, 21, 0, {}, names(GEMM.format("full", "lds", " split"), "g0", R32P, 24)),
    ("mfma24-pad", "sym", 3, 22, 6, 0, {}, names(MF.format(24, "padded", "two-images"), "g0", R32P, 22)),
    ("mfma24-pad-single", "sym", 2, 23, 17, 0, {}, names(MF.format(24, "padded", "one-image"), "g0", R32P, 23)),
    # complex order 12: folded up to m + 1 = 16 and from 25, full form at 17 .. 21, the GEMM beyond
    ("c12-folded", "herm", 3, 12, 8, 2, {}, names("lmi_schur_mfma<24,folded> two-images", "g0", T24E, 24)),
    ("c12-folded-single", "herm", 2, 12, 29, 2, {}, names("lmi_schur_mfma<24,folded> one-image", "g0", T24E, 24)),
    ("c12-m18-full", "herm", 2, 12, 18, 2, {}, names(MF.format(24, "exact", "one-image"), "g0", T24E, 24)),
    ("c12-m22", "herm", 2, 12, 22, 2, {}, names(GEMM.format("folded", "lds", " split"), "g0", T24E, 24)),
    ("c5", "herm", 3, 5, 4, 2, {}, names(MF.format(12, "padded", "two-images"), "g0", T24P, 10)),
    ("h3", "herm", 2, 3, 3, 4, {}, names(MF.format(12, "exact", "two-images"), "g0", T24P, 12)),
    # the padded Taylor instance: real-representation orders 25 .. 31
    ("c13", "herm", 3, 13, 5, 2, {}, names(GEMM.format("folded", "lds", " split"), "g0", T32P, 26)),
    ("c13-one-split", "herm", 2, 13, 5, 2, ONE, names(GEMM.format("folded", "lds", ""), "g0", T32P, 26)),
    ("c13-no-fold", "herm", 2, 13, 5, 2, {"CXK_NO_HERM_FOLD": "1"}, names(GEMM.format("full", "lds", " split"), "g0", T32P, 26)),
    ("c15", "herm", 2, 15, 4, 2, {}, names(GEMM.format("folded", "lds", " split"), "g0", T32P, 30)),
    ("h8", "herm", 2, 8, 4, 4, {}, names(GEMM.format("folded", "lds", " split"), "g0", T32E, 32)),
    ("n32", "sym", 2, 32, 6, 0, {}, names(GEMM.format("full", "lds", " split"), "g0", R32E, 32)),
    # the LDS edge: order 63 on the LDS kernels (158 760 B), 64 on the HBM path
    ("n63", "sym", 2, 63, 4, 0, {}, names(GEMM.format("full", "lds", " split"), "g0", "lmi_take_step_generic<0>", 63)),
    ("n64", "sym", 2, 64, 4, 0, {}, names(GEMM.format("full", "large", " split"), "large", "LmiLargeTakeStep pade", 64, True)),
    ("n64-one-split", "sym", 2, 64, 3, 0, ONE, names(GEMM.format("full", "large", ""), "large", "LmiLargeTakeStep pade", 64, True)),
    ("h16", "herm", 2, 16, 3, 4, {}, names(GEMM.format("folded", "large", " split"), "large", "LmiLargeTakeStep taylor", 64, True)),
    ("c32-one-split", "herm", 2, 32, 3, 2, ONE, names(GEMM.format("folded", "large", ""), "large", "LmiLargeTakeStep taylor", 64, True)),
    # prepare / query edges: rows kernel up to m = 64, packed slack or not, the LDS kernel by request
    ("n20-m64", "sym", 2, 20, 64, 0, {}, names(GEMM.format("full", "lds", " split"), "rows-packed", R20E, 20)),
    ("n20-m65", "sym", 2, 20, 65, 0, {}, names(GEMM.format("full", "lds", " split"), "g20", R20E, 20)),
    ("n20-unpacked", "sym", 3, 20, 12, 0, {"CXK_NO_PACKED_SLACK": "1"}, names(MF.format(20, "exact", "two-images"), "rows-unpacked", R20E, 20)),
    ("n20-prepare-lds", "sym", 2, 20, 12, 0, {"CXK_PREPARE_LDS": "1"}, names(MF.format(20, "exact", "two-images"), "g20", R20E, 20)),
    ("n7-prepare-lds", "sym", 2, 7, 5, 0, {"CXK_PREPARE_LDS": "1"}, names(MF.format(8, "padded", "two-images"), "g0", R20P, 7)),
    ("gemm-min-n", "sym", 2, 10, 40, 0, {"CXK_GEMM_MIN_N": "12"}, names("lmi_schur_generic symmetric", "even", R20P, 10)),
    # sparse evaluation
    ("sparse-small", "sparse", 3, 12, 6, 0, {"CXK_SPARSE_LMI": "1"}, names("lmi_schur_sparse small", "g0", R20P, 12)),
    ("sparse-small-dense-c", "sparse-densec", 2, 12, 6, 0, {"CXK_SPARSE_LMI": "1"}, names("lmi_schur_sparse small dense-C", "g0", R20P, 12)),
    ("sparse-hbm", "sparse", 2, 64, 3, 0, {"CXK_SPARSE_LMI": "1"}, names("lmi_schur_sparse hbm", "large", "LmiLargeTakeStep pade", 64, True)),
    ("sparse-hbm-dense-c", "sparse-densec", 2, 64, 3, 0, {"CXK_SPARSE_LMI": "1"}, names("lmi_schur_sparse hbm dense-C", "large", "LmiLargeTakeStep pade", 64, True)),
]

def make_problem(kind, K, n, m, d, seed):
    rng = np.random.default_rng(seed)
    if kind == "herm":
        prob = syn.hermitian_problem(K=K, n=n, d=d, m=m, branching=2, overlap=min(2, m), seed=seed)
    else:
        prob = syn.lmi_problem(K=K, n=n, m=m, branching=2, overlap=min(2, m), seed=seed)
        if kind == "nonsym":
            prob["A"] = rng.uniform(-1, 1, prob["A"].shape)
        if kind.startswith("sparse"):
            prob = syn.sparsify(prob, 0.08, seed=seed + 1)
        if kind == "sparse-densec":
            for c in range(K):
                R = syn.random_sym(rng, n)
                prob["C"][c] = np.eye(n) + 0.2 * R / np.linalg.norm(R, 2)
    return prob


def slack_norm(A, y, d):
    """||sum_i y_i A_i||_2 of one constraint."""
    S = np.tensordot(y, A, axes=1)
    return np.linalg.norm(ref.complex_rep(S, max(d, 1)) if d else S, 2)


def scaling_points(point, K, n, d, seed):
    if point == "well":
        return syn.hermitian_scaling_points(K, n, d, seed=seed) if d else syn.scaling_points(K, n, seed=seed, scale=0.3)
    rng = np.random.default_rng(seed)
    if d:
        return np.stack([ref.ill_conditioned_hermitian_W(rng, n, d, point) for _ in range(K)])
    return np.stack([ref.ill_conditioned_W(rng, n, point) for _ in range(K)])


def within(gpu, val, mag, c, what):
    gpu = np.asarray(gpu, dtype=np.float64)
    err = np.abs(gpu.astype(ref.LD) - val)
    bound = c * U * mag
    worst = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
    assert np.all(err <= bound), f"{what}: error {worst:.3g} x the bound c u |.| (c = {c})"


def sample(K):
    if K <= 8:
        return list(range(K))
    return sorted({0, 1, K // 2, K - 2, K - 1, 255, 256} & set(range(K)))


def lanczos_determined(A, Cm, W, z, dd, point, spec):
    """Per constraint: is the Lanczos run of the query / of PrepareStep determined by its input?

    Past the point where the unreorthogonalised recurrence turns into rounding noise, a change of WS in
    the last bit moves the non-dominant Ritz value anywhere (ref.ritz_spread): the oracle and the device,
    which sum in different orders, then agree only by chance, and either may leave the spectrum.  Real
    data: measured by float64 runs of the reference's recurrence.  Hermitian data (its random start
    vector and relative break are not restated here): the well-conditioned points only."""
    K = len(z)
    if dd:
        return [point == "well"] * K, [point == "well"] * K
    stable_q, stable_p = [], []
    for c in range(K):
        WS, _, S = ref.weighted_slack(A[c], Cm[c], W[c], z[c], C_WEIGHT, 0)
        WS, S = np.asarray(WS[0], dtype=np.float64), np.asarray(S[0], dtype=np.float64)
        n = WS.shape[0]
        idx = int(np.argmax(np.diag(WS)))
        bar = STABLE * max(abs(spec[c][0]), abs(spec[c][1]))
        stable_q.append(ref.ritz_spread(WS, W[c], S[:, idx], n // 2) <= bar)  # (the query starts from minus_s)
        stable_p.append(ref.ritz_spread(WS, W[c], WS[:, idx], n // 2) <= bar)
    return stable_q, stable_p


def run_point(prob, kind, d, point, seed, expected, tied=False):
    K, n = len(prob["cliques"]), prob["n"]
    herm = kind == "herm"
    A, Cm = prob["A"], prob["C"]
    W = scaling_points(point, K, n, d, seed)
    if tied:
        W = np.broadcast_to(np.eye(n), (K, n, n)).copy()
    o = syn.build(ol.Program, prob, "herm" if herm else "lmi")
    k = syn.build(KktContext, prob, "herm" if herm else "lmi", device=0)
    for i in range(K):
        o.set_W(i, W[i])
        k.set_W(i, W[i])
    for i in range(K):
        got = k.lmi_kernels(i)
        assert got == expected, f"constraint {i}: {got}"
    # y with S = C - sum y_i A_i positive definite for every constraint (||sum y_i A_i|| <= 0.5)
    rng = np.random.default_rng(seed + 1)
    y = rng.uniform(-1, 1, o.N)
    y *= 0.5 / max(slack_norm(A[c], y[cl], d) for c, cl in enumerate(prob["cliques"]))
    z = [y[cl] for cl in prob["cliques"]]
    dd = d if herm else 0
    cols = lambda X: np.asarray(X, dtype=np.float64).T if dd == 0 else np.asarray(X, dtype=np.float64)  # noqa: E731
    picks = sample(K)

    # Schur complement
    k.assemble()
    for i in picks:
        r = ref.schur(A[i], Cm[i], W[i], dd)
        Gk, AWk, AQk, sck = k.constraint_schur(i)
        low = np.tril(np.ones_like(Gk, dtype=bool))
        within(Gk[low], r["G"][0][low], r["G"][1][low], C_SCHUR, f"G of constraint {i}")
        within(AWk, *r["AW"], C_SCHUR, f"AW of constraint {i}")
        within(AQk, *r["AQc"], C_SCHUR, f"AQc of constraint {i}")
        within(sck, *r["sc"], C_SCHUR, f"<C, W>, <C, WCW> of constraint {i}")

    # the eigenvalue query: frob and trace summed over the constraints, Ritz values in the spectrum
    ek = k.weighted_slack_eigenvalues(y, C_WEIGHT)
    eo = o.weighted_slack_eigenvalues(y, C_WEIGHT)
    preps = [ref.prepare(A[c], Cm[c], W[c], z[c], C_WEIGHT, dd) for c in range(K)]
    within(ek[2], sum(p["frob"][0] for p in preps), sum(p["frob"][1] for p in preps), C_PREPARE, "query frob")
    within(ek[3], sum(p["trace"][0] for p in preps), sum(p["trace"][1] for p in preps), C_PREPARE, "query trace")
    symmetric = kind != "nonsym"
    checked = dict(query=False, prepare=0)
    if symmetric:
        spec = [ref.slack_spectrum(A[c], Cm[c], W[c], z[c], C_WEIGHT, dd) for c in range(K)]
        rho = max(max(abs(lo), abs(hi)) for lo, hi in spec)
        lo_all, hi_all = min(s[0] for s in spec), max(s[1] for s in spec)
        width = hi_all - lo_all
        # lmax comes from the dominant end of the spectrum, which every run has converged to: always
        # against the oracle; in the spectrum (and lmin, the other end, too) wherever the runs are
        # determined by their input -- rounding noise moves even the converged end by ~1e-6 of it
        assert abs(ek[1] - eo[1]) <= TOL_LANCZOS * rho, (ek, eo)
        assert ek[0] <= ek[1]
        stable_q, stable_p = lanczos_determined(A, Cm, W, z, dd, point, spec)
        if all(stable_q):
            assert -hi_all - TOL_SPECTRUM * rho <= ek[1] <= -lo_all + TOL_SPECTRUM * rho, (ek, spec)
            assert -hi_all - TOL_SPECTRUM * rho <= ek[0] <= -lo_all + TOL_SPECTRUM * rho, (ek, spec)
            assert abs(ek[0] - eo[0]) <= TOL_LANCZOS * width, (ek, eo)
            checked["query"] = True

    # PrepareStep, then TakeStep at the usual step and at one with ||X|| ~ 1
    WS1 = [np.asarray(ref.weighted_slack(A[c], Cm[c], W[c], z[c], C_WEIGHT, dd)[0], dtype=np.float64) for c in range(K)]
    for ws in WS1:
        ws[0] += np.eye(n)
    xnorm = max(np.linalg.norm(ref.complex_rep(ws, max(dd, 1)), 2) for ws in WS1)
    for which in (0, 1):
        if which:
            for i in range(K):
                o.set_W(i, W[i])
                k.set_W(i, W[i])
        ik = k.prepare_step(y, C_WEIGHT, 1.0)
        io = o.prepare_step(y, C_WEIGHT, 1.0)
        info = k.step_info()
        for c in picks:
            within(info[c, 0], *preps[c]["normsqrd"], C_PREPARE, f"normsqrd of constraint {c}")
            if symmetric and stable_p[c]:
                lo, hi = spec[c]
                assert info[c, 1] <= max(abs(1 + lo), abs(1 + hi)) + TOL_SPECTRUM * max(abs(lo), abs(hi))
                checked["prepare"] += 1
        if symmetric and all(stable_p):
            assert abs(ik[1] - io[1]) <= TOL_LANCZOS * max(width, abs(io[1])), (ik, io)
        step = min(1.0, 2.0 / ik[1] ** 2) if which == 0 else 1.0 / xnorm
        k.take_step(step, 1.0)
        o.take_step(step, 1.0)
        for c in picks:
            Wn, Wm, growth = ref.take_step(A[c], Cm[c], W[c], z[c], C_WEIGHT, 1.0, step, dd)
            within(k.get_W(c).reshape(np.shape(Wn)), cols(Wn), cols(Wm), C_TAKE * growth,
                   f"W after the step {step:.3g} of constraint {c}")

    # the affine update
    for i in range(K):
        k.set_W(i, W[i])
    k.prepare_step(y, C_WEIGHT, 0.3, affine=1)
    for c in picks:
        Wa, Wm = ref.affine(A[c], Cm[c], W[c], z[c], C_WEIGHT, 0.3, dd)
        within(k.get_W(c).reshape(np.shape(Wa)), cols(Wa), cols(Wm), C_AFFINE, f"affine W of constraint {c}")
    return checked


def set_switches(monkeypatch, env):
    for v in ("CXK_SPARSE_LMI", "CXK_LMI_SCHUR", "CXK_GEMM_MIN_N", "CXK_NO_PACKED_SLACK", "CXK_NO_HERM_FOLD",
              "CXK_PREPARE_LDS", "CXK_GRAM_SPLITS"):
        monkeypatch.delenv(v, raising=False)
    for key, val in env.items():
        monkeypatch.setenv(key, val)


@pytest.mark.parametrize("point", POINTS, ids=lambda p: p if isinstance(p, str) else f"cond{p:.0e}")
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_lmi_kernel_matrix(case, point, monkeypatch):
    cid, kind, K, n, m, d, env, expected = case
    set_switches(monkeypatch, env)
    seed = 1000 + 37 * n + m + d + K
    prob = make_problem(kind, K, n, m, d, seed)
    run_point(prob, kind, d, point, seed + 5, expected)


@pytest.mark.parametrize("n", [13, 20, 30])
def test_tied_diagonal_takes_the_first_maximum(n, monkeypatch):
    """W = I, C = I and A_i with a zero diagonal: every diagonal entry of WS ties, and the Lanczos
    start is the first column (the oracle's argmax_diag), so the Ritz values match the oracle's."""
    set_switches(monkeypatch, {})
    prob = syn.lmi_problem(K=2, n=n, m=5, branching=2, overlap=2, seed=90 + n)
    for c in range(2):
        for i in range(5):
            np.fill_diagonal(prob["A"][c, i], 0.0)
    expected = {20: names(MF.format(20, "exact", "two-images"), "rows-packed", R20E, 20),
                13: names(MF.format(16, "padded", "two-images"), "odd", R20P, 13),
                30: names(GEMM.format("full", "lds", " split"), "g0", R32P, 30)}[n]
    checked = run_point(prob, "sym", 0, "well", 91 + n, expected, tied=True)
    assert checked["query"] and checked["prepare"] == 4


def test_every_instance_has_a_case():
    """The rows name every instance the library can report (and each row asserts what it ran)."""
    listed = {name for case in CASES for name in case[-1].values()}
    assert set(lmi_kernel_names()) == listed, sorted(set(lmi_kernel_names()) ^ listed)
