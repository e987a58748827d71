"""LMIs given by factors, without a GPU: the float64 evidence for the bounds of test_gpu_lmi_factored.py, the
host-only context, the program layer and the generator.

Evidence: the factored expressions of kernels_lmi_factored.hip.h evaluated in float64 numpy in the kernels'
summation orders (lmi_factored_cases.model_*), on every row and every scaling point of the GPU test, lie within the
bounds that test asserts -- measured between 8e-6 and 0.16 of them (the worst: the affine update of the R = 129
row; G 0.063, AW 0.026, AQc 0.029, the scalars 0.028, normsqrd 0.011, frob 0.022, trace 0.028, TakeStep 0.0067).
"""
import ctypes as C

import numpy as np
import pytest

import lmi_factored_cases as fc
from conex_amd import KktContext, capi, lmi_kernel_names
from conex_amd import synthetic as syn
from conex_amd.kkt import KktError, _dp, _ip
from test_gpu_lmi_kernel_matrix import C_AFFINE, C_PREPARE, C_SCHUR, C_TAKE, C_WEIGHT, CASES, POINTS

POINT_IDS = [p if isinstance(p, str) else f"cond{p:.0e}" for p in POINTS]


# ------------------------------------------------------------------------------------ float64 evidence
@pytest.mark.parametrize("point", POINTS, ids=POINT_IDS)
@pytest.mark.parametrize("row", list(fc.ROWS))
def test_float64_in_the_kernels_order_is_within_the_bounds(row, point):
    prob = fc.make_row(row)
    seed = 31 + list(fc.ROWS).index(row)
    W = fc.points(prob, point, seed)
    y = fc.direction(prob, seed)
    n = prob["n"]
    worst = {}
    for c, cl in enumerate(prob["cliques"]):
        F, ptr, sg, Cm, z = prob["F"][c], prob["rank_ptr"][c], prob["sigma"][c], prob["C"][c], y[cl]
        G, AW, AQ, sc = fc.model_schur(F, ptr, sg, Cm, W[c])
        r = fc.ref_schur(prob, c, W[c])
        low = np.tril(np.ones_like(G, dtype=bool))
        worst["G"] = fc.ratio(G[low], r["G"][0][low], r["G"][1][low], C_SCHUR)
        worst["AW"] = fc.ratio(AW, *r["AW"], C_SCHUR)
        worst["AQc"] = fc.ratio(AQ, *r["AQc"], C_SCHUR)
        worst["scalars"] = fc.ratio(sc, *r["sc"], C_SCHUR)
        for v in np.flatnonzero(np.diff(ptr) == 0):  # an empty variable: exact zeros
            assert not G[v, :v + 1].any() and not G[v:, v].any() and AW[v] == 0.0 and AQ[v] == 0.0
        S = fc.model_slack(F, ptr, sg, Cm, z, C_WEIGHT)
        p = fc.ref_prepare(prob, c, W[c], z)
        n2, frob, tr, _, WS = fc.model_step(S, W[c], 1.0, 1.0)
        worst["normsqrd"] = fc.ratio(n2, *p["normsqrd"], C_PREPARE)
        worst["frob"] = fc.ratio(frob, *p["frob"], C_PREPARE)
        worst["trace"] = fc.ratio(tr, *p["trace"], C_PREPARE)
        for step in (0.5, 1.0 / np.linalg.norm(WS + np.eye(n), 2)):
            Wn, Wm, growth = fc.ref_take_step(prob, c, W[c], z, 1.0, step)
            worst[f"take {step:.2g}"] = fc.ratio(fc.model_step(S, W[c], 1.0, step)[3], Wn, Wm, C_TAKE * growth)
        Wa, Wm = fc.ref_affine(prob, c, W[c], z, 0.3)
        worst["affine"] = fc.ratio(fc.model_affine(WS, W[c], 0.3), Wa, Wm, C_AFFINE)
        print(row, point, c, {k: float(f"{v:.3g}") for k, v in worst.items()})
        assert all(v <= 1.0 for v in worst.values()), worst


# ------------------------------------------------------------------------------------ generator
def test_the_generator_expands_to_exactly_the_matrices_it_reports():
    for row in ("n13-three-members", "n12-theta-pairs", "n5-ranks-1-2-0"):
        prob = fc.make_row(row)
        for c in range(len(prob["cliques"])):
            F, ptr, sg = prob["F"][c], prob["rank_ptr"][c], prob["sigma"][c]
            for i in range(prob["m"]):
                want = np.zeros((prob["n"], prob["n"]))
                for k in range(ptr[i], ptr[i + 1]):
                    want += sg[k] * np.outer(F[:, k], F[:, k])
                assert np.array_equal(prob["A"][c, i], want) and np.array_equal(want, want.T)
            assert np.linalg.eigvalsh(prob["C"][c]).min() > 0
    prob = fc.make_row("n5-ranks-1-2-0")
    assert not prob["A"][0, 2].any() and prob["rank_ptr"][0].tolist() == [0, 1, 3, 3]
    lmi = syn.lmi_problem(K=3, n=12, m=8, branching=2, overlap=2, seed=1)
    fac = syn.factored_lmi_problem(K=3, n=12, ranks=(1,) * 8, branching=2, overlap=2, seed=1)
    assert fac["cliques"] == lmi["cliques"] and fac["num_vars"] == lmi["num_vars"]  # the same clique tree
    # b = sum_c <A_ci, X_c> with X_c positive definite: every b_i of a positive semidefinite A_i alone is positive
    assert np.all(fac["b"] > 0)


# ------------------------------------------------------------------------------------ host-only context
def host_context(prob):
    k = KktContext(prob["num_vars"], device=-1)
    for c, cl in enumerate(prob["cliques"]):
        assert k.add_lmi_factored(prob["F"][c], prob["rank_ptr"][c], prob["sigma"][c], prob["C"][c], cl) == c
    return k


def test_a_host_only_context_takes_factored_constraints():
    prob = fc.make_row("n13-three-members")
    k = host_context(prob)
    assert k.count_factored_lmi() == -1  # not finalized yet
    k.initialize()
    assert k.count_factored_lmi() == 3   # (a property of how they were added, as cxk_count_sparse_lmi counts there)
    assert [k.L.cxk_dual_size(k.h, i) for i in range(3)] == [13 * 13] * 3
    assert k.N == prob["num_vars"] and k.K == 3
    with pytest.raises(KktError):
        k.lmi_kernels(0)
    # the reported instances are the rows of the LMI matrix, no more: the route adds no name
    assert set(lmi_kernel_names()) == {name for case in CASES for name in case[-1].values()}
    byt, flops = k.assembly_work()
    dense = KktContext(prob["num_vars"], device=-1)
    for c, cl in enumerate(prob["cliques"]):
        dense.add_lmi(prob["A"][c], prob["C"][c], cl)
    dense.initialize()
    byt0, flops0 = dense.assembly_work()
    assert 0 < flops < flops0 and 0 < byt  # (the route's own count: at n = m = R = 13 already below the dense formula)


def raw_add(k, n, m, ptr, F, sigma, Cm):
    ptr = None if ptr is None else np.ascontiguousarray(ptr, dtype=np.int32)
    F = None if F is None else np.ascontiguousarray(F, dtype=np.float64)
    sigma = None if sigma is None else np.ascontiguousarray(sigma, dtype=np.float64)
    Cm = None if Cm is None else np.ascontiguousarray(Cm, dtype=np.float64)
    r = k.L.cxk_add_lmi_factored(k.h, n, m, None if ptr is None else _ip(ptr), None if F is None else _dp(F),
                                 None if sigma is None else _dp(sigma), None if Cm is None else _dp(Cm), None)
    return r, k.L.cxk_last_error(k.h).decode()


@pytest.mark.parametrize("what,message", [
    ("n", "n is at least 1 and m at least 0"), ("m", "n is at least 1 and m at least 0"),
    ("null-ptr", "rank_ptr or C is null"), ("null-C", "rank_ptr or C is null"), ("null-F", "F is null"),
    ("start", r"rank_ptr\[0\] is not 0"), ("decreasing", "rank_ptr decreases"),
    ("nan-F", "F holds a value that is not finite"), ("inf-sigma", "sigma holds a value that is not finite"),
    ("nan-C", "C holds a value that is not finite"), ("unsymmetric", "C is not symmetric"),
])
def test_refusals_at_the_call(what, message):
    import re
    n, m = 3, 2
    ptr, F, sg, Cm = [0, 1, 3], np.ones((3, 3)), np.ones(3), np.eye(3)
    k = KktContext(m, device=-1)
    if what == "n":
        n = 0
    elif what == "m":
        m = -1
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
        F[1, 1] = np.nan
    elif what == "inf-sigma":
        sg = np.array([1.0, np.inf, 1.0])
    elif what == "nan-C":
        Cm = Cm.copy()
        Cm[2, 2] = np.nan
    elif what == "unsymmetric":
        Cm = Cm.copy()
        Cm[0, 1] = 0.5
    r, err = raw_add(k, n, m, ptr, F, sg, Cm)
    assert r == -1 and re.search("cxk_add_lmi_factored: " + message, err), err
    assert raw_add(k, 3, 2, [0, 1, 3], np.ones((3, 3)), None, np.eye(3))[0] == 0  # (sigma NULL: all +1; the context lives on)


def test_refusals_at_finalize():
    k = KktContext(1, device=-1)
    assert k.add_lmi_factored(np.ones((1025, 1)), [0, 1], None, np.eye(1025)) == 0
    with pytest.raises(KktError, match="order above 1024"):
        k.initialize()
    k = KktContext(1, device=-1)
    R = 46341  # R * R = 2 147 488 281 > INT_MAX
    assert k.add_lmi_factored(np.zeros((1, R)), [0, R], None, np.eye(1)) == 0
    with pytest.raises(KktError, match="n x R, R x R or m x m entries exceed the int range"):
        k.initialize()
    m = 46341
    k = KktContext(m, device=-1)
    assert k.add_lmi_factored(np.zeros((1, 0)), np.zeros(m + 1, dtype=np.int32), None, np.eye(1)) == 0
    with pytest.raises(KktError, match="exceed the int range"):
        k.initialize()


def test_the_wrapper_checks_its_shapes():
    k = KktContext(2, device=-1)
    with pytest.raises(ValueError, match="add_lmi_factored"):
        k.add_lmi_factored(np.ones((3, 3)), [0, 1, 2], None, np.eye(3))       # rank_ptr does not end at R
    with pytest.raises(ValueError, match="add_lmi_factored"):
        k.add_lmi_factored(np.ones((3, 3)), [0, 1, 3], np.ones(2), np.eye(3))  # sigma of the wrong length


# ------------------------------------------------------------------------------------ program layer
def test_the_new_symbols_are_exported():
    L = KktContext(1, device=-1).L
    for name in ("cxk_add_lmi_factored", "cxk_count_factored_lmi"):
        assert getattr(L, name).argtypes is not None
    assert capi.api().CONEX_HIP_AddFactoredLMIConstraint.argtypes is not None


def test_program_layer_ids_bad_arguments_and_updates():
    A = capi.api()
    p = A.CONEX_CreateConeProgram()
    assert A.CONEX_SetNumberOfVariables(p, 3) == 0
    n, R = 4, 4
    F = np.ascontiguousarray(np.random.default_rng(1).standard_normal(n * R))
    sg = np.array([1.0, -1.0, 1.0, 1.0])
    ptr = np.array([0, 1, 3, 4], dtype=np.int32)
    Cm = np.ascontiguousarray(np.eye(n).ravel())
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_long))  # noqa: E731
    add = A.CONEX_HIP_AddFactoredLMIConstraint
    assert add(p, n, capi.dp(F), R, capi.dp(sg), ip(ptr), 3, capi.dp(Cm), None) == 0
    two = np.array([2, 0], dtype=np.int64)
    ptr2 = np.array([0, 2, 4], dtype=np.int32)
    assert add(p, n, capi.dp(F), R, None, ip(ptr2), 2, capi.dp(Cm), lp(two)) == 1
    assert A.CONEX_GetDualVariableSize(p, 0) == n * n and A.CONEX_GetDualVariableSize(p, 1) == n * n
    bad_start = np.array([1, 1, 3, 4], dtype=np.int32)
    decreasing = np.array([0, 3, 1, 4], dtype=np.int32)
    short = np.array([0, 1, 2, 3], dtype=np.int32)
    Fnan = F.copy()
    Fnan[5] = np.nan
    Cun = Cm.copy()
    Cun[1] = 0.25
    outside = np.array([0, 7], dtype=np.int64)
    for args in ((None, n, capi.dp(F), R, capi.dp(sg), ip(ptr), 3, capi.dp(Cm), None),      # no program
                 (p, 0, capi.dp(F), R, capi.dp(sg), ip(ptr), 3, capi.dp(Cm), None),         # n < 1
                 (p, n, None, R, capi.dp(sg), ip(ptr), 3, capi.dp(Cm), None),               # F null
                 (p, n, capi.dp(F), R, capi.dp(sg), None, 3, capi.dp(Cm), None),            # rank_ptr null
                 (p, n, capi.dp(F), R, capi.dp(sg), ip(ptr), 3, None, None),                # c null
                 (p, n, capi.dp(F), R, capi.dp(sg), ip(ptr2), 2, capi.dp(Cm), None),        # not every variable, no list
                 (p, n, capi.dp(F), R, capi.dp(sg), ip(bad_start), 3, capi.dp(Cm), None),   # rank_ptr[0] != 0
                 (p, n, capi.dp(F), R, capi.dp(sg), ip(decreasing), 3, capi.dp(Cm), None),  # decreasing
                 (p, n, capi.dp(F), R, capi.dp(sg), ip(short), 3, capi.dp(Cm), None),       # does not end at R
                 (p, n, capi.dp(Fnan), R, capi.dp(sg), ip(ptr), 3, capi.dp(Cm), None),      # not finite
                 (p, n, capi.dp(F), R, capi.dp(sg), ip(ptr), 3, capi.dp(Cun), None),        # c not symmetric
                 (p, n, capi.dp(F), R, capi.dp(sg), ip(ptr2), 2, capi.dp(Cm), lp(outside))):  # a variable out of range
        assert add(*args) == -1
    assert A.CONEX_UpdateLinearOperator(p, 0, 1.0, 0, 0, 0, 0) != 0
    assert A.CONEX_UpdateAffineTerm(p, 1, 1.0, 0, 0, 0) != 0
    A.CONEX_DeleteConeProgram(p)
