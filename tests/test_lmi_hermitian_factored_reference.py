"""Hermitian matrix inequalities given by factors, without a GPU: the float64 evidence for the bounds of
test_gpu_lmi_hermitian_factored.py, the folded identities, the host-only context, the program layer and the generator.

Evidence: the folded expressions of kernels_lmi_factored.hip.h evaluated in float64 numpy in the kernels' summation
orders (lmi_hermitian_factored_cases.model_*), on every row and every scaling point of the GPU test, lie within the
bounds that test asserts (each case prints its ratios to the bounds).
"""
import ctypes as C
import re

import numpy as np
import pytest

import lmi_hermitian_factored_cases as hc
import lmi_reference as ref
from conex_amd import KktContext, capi, lmi_kernel_names
from conex_amd import synthetic as syn
from conex_amd.kkt import KktError, _dp, _ip
from test_gpu_lmi_kernel_matrix import C_AFFINE, C_PREPARE, C_SCHUR, C_TAKE, C_WEIGHT, CASES, POINTS

POINT_IDS = [p if isinstance(p, str) else f"cond{p:.0e}" for p in POINTS]


# ------------------------------------------------------------------------------------ float64 evidence
@pytest.mark.parametrize("point", POINTS, ids=POINT_IDS)
@pytest.mark.parametrize("row", list(hc.ROWS))
def test_float64_in_the_kernels_order_is_within_the_bounds(row, point):
    prob = hc.make_row(row)
    seed = hc.row_seed(row)
    W = hc.points(prob, point, seed)
    y = hc.direction(prob, seed)
    d = prob["d"]
    worst = {}
    for c, cl in enumerate(prob["cliques"]):
        F, ptr, sg, Cm, z = prob["F"][c], prob["rank_ptr"][c], prob["sigma"][c], prob["C"][c], y[cl]
        G, AW, AQ, sc = hc.model_schur(F, ptr, sg, Cm, W[c])
        r = hc.ref_schur(prob, c, W[c])
        low = np.tril(np.ones_like(G, dtype=bool))
        worst["G"] = hc.ratio(G[low], r["G"][0][low], r["G"][1][low], C_SCHUR)
        worst["AW"] = hc.ratio(AW, *r["AW"], C_SCHUR)
        worst["AQc"] = hc.ratio(AQ, *r["AQc"], C_SCHUR)
        worst["scalars"] = hc.ratio(sc, *r["sc"], C_SCHUR)
        for v in np.flatnonzero(np.diff(ptr) == 0):  # an empty variable: exact zeros
            assert not G[v, :v + 1].any() and not G[v:, v].any() and AW[v] == 0.0 and AQ[v] == 0.0
        S = hc.model_slack(F, ptr, sg, Cm, z, C_WEIGHT)
        p = hc.ref_prepare(prob, c, W[c], z)
        n2, frob, tr, _, WS = hc.model_step(S, W[c], 1.0, 1.0)
        worst["normsqrd"] = hc.ratio(n2, *p["normsqrd"], C_PREPARE)
        worst["frob"] = hc.ratio(frob, *p["frob"], C_PREPARE)
        worst["trace"] = hc.ratio(tr, *p["trace"], C_PREPARE)
        for step in (0.5, 1.0 / np.linalg.norm(WS + np.eye(len(WS)), 2)):
            Wn, Wm, growth = hc.ref_take_step(prob, c, W[c], z, 1.0, step)
            worst[f"take {step:.2g}"] = hc.ratio(hc.model_step(S, W[c], 1.0, step)[3], Wn, Wm, C_TAKE * growth)
        Wa, Wm = hc.ref_affine(prob, c, W[c], z, 0.3)
        worst["affine"] = hc.ratio(hc.model_affine(WS, W[c], 0.3), Wa, Wm, C_AFFINE)
        print(row, point, c, {k: float(f"{v:.3g}") for k, v in worst.items()})
        assert all(v <= 1.0 for v in worst.values()), worst
        assert d == F.shape[0]


# ------------------------------------------------------------------------------------ the folded identities
@pytest.mark.parametrize("d", [1, 2, 4])
def test_the_folded_identities_hold_against_the_expansion(d):
    """L(f f^*) = L(f) L(f)', P_0 symmetric and the other planes skew, and G, AW, AQc, S of the folded form equal those
    of the expanded planes (lmi_reference with its d argument) to rounding."""
    prob = syn.factored_hermitian_problem(K=1, n=5, d=d, ranks=(2, 1, 0, 1), signs="mixed", seed=3)
    F, ptr, sg, Cm, A = prob["F"][0], prob["rank_ptr"][0], prob["sigma"][0], prob["C"][0], prob["A"][0]
    W = syn.hermitian_scaling_points(1, 5, d, seed=4)[0]
    LF = hc.embed(F)
    R = F.shape[2]
    var = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    for i in range(prob["m"]):
        cols = np.flatnonzero(np.tile(var == i, d))
        assert np.allclose(hc.embed(A[i]), (LF[:, cols] * np.tile(sg, d)[cols]) @ LF[:, cols].T, atol=1e-13)
    assert np.array_equal(LF[:, :R], np.concatenate(list(F)))  # column block 0: the stacked planes
    _, _, P = hc.model_products(F, W)
    assert np.allclose(P[0], P[0].T, atol=1e-13) and all(np.allclose(P[p], -P[p].T, atol=1e-13) for p in range(1, d))
    G, AW, AQ, sc = hc.model_schur(F, ptr, sg, Cm, W)
    r = ref.schur(A, Cm, W, d)
    low = np.tril(np.ones_like(G, dtype=bool))
    for got, key in ((G[low], "G"), (AW, "AW"), (AQ, "AQc"), (sc, "sc")):
        want = np.asarray(r[key][0], dtype=np.float64)
        want = want[low] if key == "G" else want
        assert np.allclose(got, want, rtol=0, atol=1e-12 * max(1.0, np.abs(want).max())), key
    z = np.array([0.3, -0.2, 0.5, 0.1])
    S = hc.model_slack(F, ptr, sg, Cm, z, 0.7)
    want = np.asarray(ref.weighted_slack(A, Cm, W, z, 0.7, d)[2], dtype=np.float64)
    assert np.allclose(S, hc.embed(want), atol=1e-13)


# ------------------------------------------------------------------------------------ generator
def test_the_generator_expands_to_hermitian_planes():
    for row in ("n5-ranks-3-1-0-2-d2", "n5-ranks-3-1-0-2-d4", "n9-d1"):
        prob = hc.make_row(row)
        d, A = prob["d"], prob["A"][0]
        assert A.shape == (prob["m"], d, prob["n"], prob["n"])
        assert np.array_equal(A[:, 0], np.swapaxes(A[:, 0], -1, -2))
        assert all(np.array_equal(A[:, p], -np.swapaxes(A[:, p], -1, -2)) for p in range(1, d))
        assert np.linalg.eigvalsh(ref.complex_rep(prob["C"][0], d)).min() > 0
    prob = hc.make_row("n5-ranks-3-1-0-2-d2")
    assert not prob["A"][0, 2].any() and prob["rank_ptr"][0].tolist() == [0, 3, 4, 4, 6]
    herm = syn.hermitian_problem(K=3, n=5, d=2, m=6, branching=2, overlap=2, seed=1)
    fac = syn.factored_hermitian_problem(K=3, n=5, d=2, ranks=(1,) * 6, branching=2, overlap=2, seed=1)
    assert fac["cliques"] == herm["cliques"] and fac["num_vars"] == herm["num_vars"]  # the same clique tree
    assert np.all(fac["b"] > 0)  # b_i = <A_i, X> with A_i positive semidefinite and X positive definite


# ------------------------------------------------------------------------------------ host-only context
def test_a_host_only_context_takes_factored_hermitian_constraints():
    prob = hc.make_row("n7-three-members-d2")
    k = KktContext(prob["num_vars"], device=-1)
    for c, cl in enumerate(prob["cliques"]):
        assert k.add_hermitian_factored(prob["F"][c], prob["rank_ptr"][c], prob["sigma"][c], prob["C"][c], cl) == c
    assert k.count_factored_lmi() == -1  # not finalized yet
    k.initialize()
    assert k.count_factored_lmi() == 3
    assert [k.L.cxk_dual_size(k.h, i) for i in range(3)] == [2 * 7 * 7] * 3  # d planes
    assert k.cons == [("herm", 7, 6, 2)] * 3
    with pytest.raises(KktError):
        k.lmi_kernels(0)
    assert set(lmi_kernel_names()) == {name for case in CASES for name in case[-1].values()}  # the route adds no name
    assert syn.build(KktContext, prob, "herm-factored", device=-1).count_factored_lmi() == 3


def test_assembly_work_reports_the_folded_counts():
    """n = m = R = 200 complex, rank one: the folded form's flops and bytes against the expanded planes through
    add_hermitian's formula (N = 400): Z and Y have R columns, not dR, and P has d R^2 entries."""
    n = m = 200
    d = 2
    rng = np.random.default_rng(0)
    k = KktContext(m, device=-1)
    Cm = np.zeros((d, n, n))
    Cm[0] = np.eye(n)
    assert k.add_hermitian_factored(rng.standard_normal((d, n, m)), np.arange(m + 1), None, Cm) == 0
    k.initialize()
    byt, flops = k.assembly_work()
    N, R = d * n, m
    terms = m * (m + 1) / 2
    assert flops == 4 * N * N * R + 2 * N * d * R * R + 4 * N ** 3 + 4 * N * N + (2 * d + 1) * terms + 2 * N * R + 2 * R
    assert byt == 8.0 * (N * R + N * d * R + 2 * N * N + 4 * N * R + N * R + d * R * R + 4 * N * N + m * (m + 1) / 2 + 2 * m + R + m)
    dense_flops = 4 * N ** 3 * (m + 1) + N * N * (m * m + 3 * m + 4) + N * m
    # below the expanded form's count, and fewer bytes than a tenth of the m (d n)^2 array alone, which nothing holds
    assert flops < dense_flops and byt < 8.0 * m * N * N / 10


def raw_add(k, n, d, m, ptr, F, sigma, Cm):
    ptr = None if ptr is None else np.ascontiguousarray(ptr, dtype=np.int32)
    F = None if F is None else np.ascontiguousarray(F, dtype=np.float64)
    sigma = None if sigma is None else np.ascontiguousarray(sigma, dtype=np.float64)
    Cm = None if Cm is None else np.ascontiguousarray(Cm, dtype=np.float64)
    r = k.L.cxk_add_hermitian_factored(k.h, n, d, m, None if ptr is None else _ip(ptr), None if F is None else _dp(F),
                                       None if sigma is None else _dp(sigma), None if Cm is None else _dp(Cm), None)
    return r, k.L.cxk_last_error(k.h).decode()


def identity_planes(d, n):
    Cm = np.zeros((d, n, n))
    Cm[0] = np.eye(n)
    return Cm


@pytest.mark.parametrize("what,message", [
    ("n", "n is at least 1 and m at least 0"), ("m", "n is at least 1 and m at least 0"),
    ("d3", "the hyper-complex dimension is 1, 2 or 4"), ("d8", "octonions have no real representation"),
    ("null-ptr", "rank_ptr or C is null"), ("null-C", "rank_ptr or C is null"), ("null-F", "F is null"),
    ("start", r"rank_ptr\[0\] is not 0"), ("decreasing", "rank_ptr decreases"),
    ("nan-F", "F holds a value that is not finite"), ("inf-sigma", "sigma holds a value that is not finite"),
    ("nan-C", "C holds a value that is not finite"), ("unsymmetric-plane0", "C is not Hermitian"),
    ("symmetric-plane1", "C is not Hermitian"), ("diagonal-plane1", "C is not Hermitian"),
])
def test_refusals_at_the_call(what, message):
    n, d, m = 3, 2, 2
    ptr, F, sg, Cm = [0, 1, 3], np.ones((2, 3, 3)), np.ones(3), identity_planes(2, 3)
    k = KktContext(m, device=-1)
    if what == "n":
        n = 0
    elif what == "m":
        m = -1
    elif what == "d3":
        d = 3
    elif what == "d8":
        d = 8
    elif what == "null-ptr":
        ptr = None
    elif what == "null-C":
        Cm = None
    elif what == "null-F":
        F = None
    elif what == "start":
        ptr = [1, 2, 3]
    elif what == "decreasing":
        ptr = [0, 2, 1]
    elif what == "nan-F":
        F = F.copy()
        F[1, 1, 1] = np.nan  # (in the second plane)
    elif what == "inf-sigma":
        sg = np.array([1.0, np.inf, 1.0])
    elif what == "nan-C":
        Cm[1, 2, 2] = np.nan
    elif what == "unsymmetric-plane0":
        Cm[0, 0, 1] = 0.5
    elif what == "symmetric-plane1":
        Cm[1, 0, 1] = Cm[1, 1, 0] = 0.5
    elif what == "diagonal-plane1":
        Cm[1, 1, 1] = 0.5
    r, err = raw_add(k, n, d, m, ptr, F, sg, Cm)
    assert r == -1 and re.search("cxk_add_hermitian_factored: .*" + message, err), err
    # (sigma NULL: all +1; the context lives on)
    assert raw_add(k, 3, 2, 2, [0, 1, 3], np.ones((2, 3, 3)), None, identity_planes(2, 3))[0] == 0


def test_refusals_at_finalize():
    k = KktContext(1, device=-1)
    n = 1275  # N = 2550: one past the largest order whose Lanczos vectors fit LDS
    assert k.add_hermitian_factored(np.ones((2, n, 1)), [0, 1], None, identity_planes(2, n)) == 0
    with pytest.raises(KktError, match=r"order above 2549 .* 163328 B of LDS"):
        k.initialize()
    k = KktContext(1, device=-1)  # (beyond cxk_add_lmi_factored's 1024, within the Hermitian limit)
    assert k.add_hermitian_factored(np.ones((2, 600, 1)), [0, 1], None, identity_planes(2, 600)) == 0
    k.initialize()
    k = KktContext(1, device=-1)
    R = 32768  # d R R = 2^31 > INT_MAX, N R and N dR within it
    assert k.add_hermitian_factored(np.zeros((2, 1, R)), [0, R], None, identity_planes(2, 1)) == 0
    with pytest.raises(KktError, match="d x R x R entries exceed the int range"):
        k.initialize()
    m = 46341
    k = KktContext(m, device=-1)
    assert k.add_hermitian_factored(np.zeros((2, 1, 0)), np.zeros(m + 1, dtype=np.int32), None, identity_planes(2, 1)) == 0
    with pytest.raises(KktError, match="m x m entries exceed the int range"):
        k.initialize()


def test_the_wrapper_checks_its_shapes():
    k = KktContext(2, device=-1)
    Cm = identity_planes(2, 3)
    with pytest.raises(ValueError, match="add_hermitian_factored"):
        k.add_hermitian_factored(np.ones((2, 3, 3)), [0, 1, 2], None, Cm)        # rank_ptr does not end at R
    with pytest.raises(ValueError, match="add_hermitian_factored"):
        k.add_hermitian_factored(np.ones((2, 3, 3)), [0, 1, 3], np.ones(2), Cm)  # sigma of the wrong length
    with pytest.raises(ValueError, match="add_hermitian_factored"):
        k.add_hermitian_factored(np.ones((3, 3)), [0, 1, 3], None, Cm)           # F is not planes
    with pytest.raises(ValueError, match="add_hermitian_factored"):
        k.add_hermitian_factored(np.ones((4, 3, 3)), [0, 1, 3], None, Cm)        # d of F and Cm differ
    with pytest.raises(ValueError, match="add_hermitian_factored"):
        k.add_hermitian_factored(np.ones((2, 3, 3)), [0, 1, 3], None, np.eye(3))  # Cm is not planes


# ------------------------------------------------------------------------------------ program layer
def test_the_new_symbols_are_exported():
    L = KktContext(1, device=-1).L
    assert L.cxk_add_hermitian_factored.argtypes is not None
    assert capi.api().CONEX_HIP_AddFactoredHermitianConstraint.argtypes is not None
    from conex_amd.program import Conex
    assert callable(Conex.AddFactoredHermitianMatrixInequality) and callable(KktContext.add_hermitian_factored)


def test_program_layer_ids_bad_arguments_and_updates():
    A = capi.api()
    p = A.CONEX_CreateConeProgram()
    assert A.CONEX_SetNumberOfVariables(p, 3) == 0
    n, d, R = 4, 2, 4
    F = np.ascontiguousarray(np.random.default_rng(1).standard_normal(d * n * R))
    sg = np.array([1.0, -1.0, 1.0, 1.0])
    ptr = np.array([0, 1, 3, 4], dtype=np.int32)
    Cm = np.ascontiguousarray(identity_planes(d, n).ravel())
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_long))  # noqa: E731
    add = A.CONEX_HIP_AddFactoredHermitianConstraint
    assert add(p, n, d, capi.dp(F), R, capi.dp(sg), ip(ptr), 3, capi.dp(Cm), None) == 0
    two = np.array([2, 0], dtype=np.int64)
    ptr2 = np.array([0, 2, 4], dtype=np.int32)
    assert add(p, n, d, capi.dp(F), R, None, ip(ptr2), 2, capi.dp(Cm), lp(two)) == 1
    Fq = np.ascontiguousarray(np.random.default_rng(2).standard_normal(4 * n * R))
    assert add(p, n, 4, capi.dp(Fq), R, None, ip(ptr), 3, capi.dp(np.ascontiguousarray(identity_planes(4, n).ravel())), None) == 2
    # the dual variable is the real plane, as for every Hermitian constraint
    assert [A.CONEX_GetDualVariableSize(p, i) for i in range(3)] == [n * n] * 3
    bad_start = np.array([1, 1, 3, 4], dtype=np.int32)
    decreasing = np.array([0, 3, 1, 4], dtype=np.int32)
    short = np.array([0, 1, 2, 3], dtype=np.int32)
    Fnan = F.copy()
    Fnan[n * R + 5] = np.nan  # (in the second plane)
    Cun = Cm.copy()
    Cun[1] = 0.25             # plane 0 not symmetric
    Csym = Cm.copy()
    Csym[n * n + 1] = Csym[n * n + n] = 0.25  # plane 1 symmetric, not skew
    outside = np.array([0, 7], dtype=np.int64)
    for args in ((None, n, d, capi.dp(F), R, capi.dp(sg), ip(ptr), 3, capi.dp(Cm), None),      # no program
                 (p, 0, d, capi.dp(F), R, capi.dp(sg), ip(ptr), 3, capi.dp(Cm), None),         # n < 1
                 (p, n, 3, capi.dp(F), R, capi.dp(sg), ip(ptr), 3, capi.dp(Cm), None),         # d not 1, 2, 4
                 (p, n, 8, capi.dp(F), R, capi.dp(sg), ip(ptr), 3, capi.dp(Cm), None),         # octonions
                 (p, n, d, None, R, capi.dp(sg), ip(ptr), 3, capi.dp(Cm), None),               # F null
                 (p, n, d, capi.dp(F), R, capi.dp(sg), None, 3, capi.dp(Cm), None),            # rank_ptr null
                 (p, n, d, capi.dp(F), R, capi.dp(sg), ip(ptr), 3, None, None),                # c null
                 (p, n, d, capi.dp(F), R, capi.dp(sg), ip(ptr2), 2, capi.dp(Cm), None),        # not every variable, no list
                 (p, n, d, capi.dp(F), R, capi.dp(sg), ip(bad_start), 3, capi.dp(Cm), None),   # rank_ptr[0] != 0
                 (p, n, d, capi.dp(F), R, capi.dp(sg), ip(decreasing), 3, capi.dp(Cm), None),  # decreasing
                 (p, n, d, capi.dp(F), R, capi.dp(sg), ip(short), 3, capi.dp(Cm), None),       # does not end at R
                 (p, n, d, capi.dp(Fnan), R, capi.dp(sg), ip(ptr), 3, capi.dp(Cm), None),      # not finite
                 (p, n, d, capi.dp(F), R, capi.dp(sg), ip(ptr), 3, capi.dp(Cun), None),        # c not Hermitian
                 (p, n, d, capi.dp(F), R, capi.dp(sg), ip(ptr), 3, capi.dp(Csym), None),       # c not Hermitian
                 (p, n, d, capi.dp(F), R, capi.dp(sg), ip(ptr2), 2, capi.dp(Cm), lp(outside))):  # a variable out of range
        assert add(*args) == -1
    assert A.CONEX_UpdateLinearOperator(p, 0, 1.0, 0, 0, 0, 0) != 0
    assert A.CONEX_UpdateAffineTerm(p, 1, 1.0, 0, 0, 0) != 0
    A.CONEX_DeleteConeProgram(p)


def test_the_program_wrapper_checks_its_shapes():
    from conex_amd.program import Conex, ConexError
    prog = Conex(2)
    Cm = identity_planes(2, 3)
    assert prog.AddFactoredHermitianMatrixInequality(np.ones((2, 3, 3)), [0, 1, 3], None, Cm) == 0
    assert prog.AddFactoredHermitianMatrixInequality(np.ones((2, 3, 1)), [0, 1], [-1.0], Cm, variables=[1]) == 1
    for F, ptr, sg, c in ((np.ones((3, 3)), [0, 1, 3], None, Cm), (np.ones((2, 3, 3)), [0, 1, 3], np.ones(2), Cm),
                          (np.ones((2, 3, 3)), [0, 3], None, Cm), (np.ones((2, 3, 3)), [0, 1, 3], None, np.eye(3))):
        with pytest.raises(ConexError):
            prog.AddFactoredHermitianMatrixInequality(F, ptr, sg, c)
