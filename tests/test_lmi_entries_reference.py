"""Matrix inequalities given by their entries, host side (no GPU): the numpy model of the restricted evaluation of the
affine term against the dense formulas in longdouble; cxk_add_lmi_coo's refusals, by their exact messages, on a
host-only context; the route and threshold functions of cone_route.h compiled alone; the program layer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lmi_entries_cases as ec
from conex_amd import KktContext, capi as ca
from conex_amd import synthetic as syn
from conex_amd.kkt import KktError, load_library
from conex_amd.program import Conex, ConexError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("n,m,nnz_c", ec.MODEL_SHAPES)
def test_restricted_evaluation_equals_the_dense_formulas(n, m, nnz_c):
    """W C W formed only where an entry reads it gives tr(A_i W C W), tr(C W C W) and tr(C W): both the restricted
    form and the float64 dense form are within the project's 1e-13 of longdouble (a scratch run of exactly this gave
    1.4e-15 and 1.2e-15 at the worst)."""
    case = ec.make_case(n, m, nnz_c, empty_a=1 if m > 2 else None)
    W = ec.symmetric_w(n)
    ref = ec.dense_formulas(case, W)
    AQc, cq, wc, npos = ec.restricted_model(case, W)
    assert ec.rel(AQc, ref["AQc"]) <= 1e-13
    assert abs(cq - ref["cq"]) <= 1e-13 * abs(ref["cq"]) and abs(wc - ref["wc"]) <= 1e-13 * abs(ref["wc"])
    f64 = ec.dense_formulas(case, W, np.float64)
    assert ec.rel(f64["AQc"], ref["AQc"]) <= 1e-13
    # the positions: every entry of the A_i and of C, both triangles, counted once
    every = {(int(c), int(r)) for i in range(m + 1) for r, c in zip(*ec.mirrored(case, i)[:2])}
    assert npos == len(every) <= np.count_nonzero(case["C"]) + sum(np.count_nonzero(a) for a in case["A"])


def test_the_model_does_not_lean_on_a_symmetric_w():
    """W is read as stored: with a W that is not symmetric the restricted form is still W C W of the dense formulas."""
    case = ec.make_case(70, 3, 90)
    rng = np.random.default_rng(4)
    W = ec.symmetric_w(70) + 0.05 * rng.standard_normal((70, 70))
    ref = ec.dense_formulas(case, W)
    AQc, cq, wc, _ = ec.restricted_model(case, W)
    assert ec.rel(AQc, ref["AQc"]) <= 1e-13 and abs(cq - ref["cq"]) <= 1e-13 * abs(ref["cq"])
    assert abs(wc - ref["wc"]) <= 1e-13 * abs(ref["wc"])


def test_the_generator_makes_what_it_says():
    c = ec.make_case(65, 3, 65, empty_index=7, empty_a=1)
    assert np.count_nonzero(c["C"]) == 65 and not c["C"][7].any() and not c["C"][:, 7].any()
    assert not c["A"][1].any() and c["ptr"][1] == c["ptr"][2]
    assert np.array_equal(c["C"], c["C"].T) and all(np.array_equal(a, a.T) for a in c["A"])
    assert np.all(c["row"] >= c["col"])
    d = ec.make_case(70, 2, 66, diag_only=True)
    assert np.count_nonzero(d["C"]) == 66 == np.count_nonzero(np.diag(d["C"]))
    on = off = 0
    for i in range(3):
        for r, cc, _ in zip(*ec.mirrored(c, i)):
            on, off = on + (c["C"][r, cc] != 0), off + (c["C"][r, cc] == 0)
    assert on > 0 and off > 0  # entries of the A_i both on and off C's pattern


def test_maxcut_entries_is_maxcut_problem():
    for n in (9, 70, 300):
        p, e = syn.maxcut_problem(n), syn.maxcut_entries(n)
        case = dict(n=n, m=n, ptr=e["ptr"], row=e["row"], col=e["col"], val=e["val"])
        C_ = np.zeros((n, n))
        r, c, v = ec.mirrored(case, n)
        C_[r, c] = v
        assert np.array_equal(C_, p["C"][0])  # the same bits: the same random stream, the same operations
        for i in (0, n // 2, n - 1):
            r, c, v = ec.mirrored(case, i)
            assert (list(r), list(c), list(v)) == ([i], [i], [-1.0])
        assert np.array_equal(e["b"], p["b"]) and e["cliques"] == p["cliques"]


# ------------------------------------------------------------------------------------ the interface, host side
def host_context(m=1):
    return KktContext(m, device=-1)


def raw_add(k, n, m, ptr, row, col, val, null=()):
    ip = lambda a: np.asarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))
    dp = lambda a: np.asarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    args = dict(ptr=ip(ptr), row=ip(row) if len(row) else ip([0]), col=ip(col) if len(col) else ip([0]),
                val=dp(val) if len(val) else dp([0.0]))
    for name in null:
        args[name] = None
    r = k.L.cxk_add_lmi_coo(k.h, n, m, args["ptr"], args["row"], args["col"], args["val"], None)
    return r, k.L.cxk_last_error(k.h).decode()


@pytest.mark.parametrize("n,m,ptr,row,col,val,message", ec.REFUSALS)
def test_add_lmi_coo_refuses_bad_input_by_name(n, m, ptr, row, col, val, message):
    k = host_context()
    r, err = raw_add(k, n, m, ptr, row, col, val)
    assert r == -1 and err == "cxk_add_lmi_coo: " + message
    assert k.L.cxk_num_constraints(k.h) == 0


def test_add_lmi_coo_refuses_null_pointers_and_too_many_variables():
    k = host_context()
    assert raw_add(k, 4, 1, [0, 1, 2], [0, 1], [0, 1], [1.0, 1.0], null=("ptr",)) == (-1, "cxk_add_lmi_coo: ptr is null")
    for name in ("row", "col", "val"):
        assert raw_add(k, 4, 1, [0, 1, 2], [0, 1], [0, 1], [1.0, 1.0], null=(name,)) == \
            (-1, "cxk_add_lmi_coo: row, col or val is null")
    assert raw_add(k, 4, 32768, [0], [], [], []) == (-1, "cxk_add_lmi_coo: " + ec.R_PACK)
    assert raw_add(k, 4, 0, [0, 0], [], [], [], null=("row", "col", "val"))[0] == -1  # m = 0 of a context of one variable
    with pytest.raises(ValueError, match="add_lmi_coo"):
        k.add_lmi_coo(4, [0, 1], [0], [0], [1.0])              # ptr too short for one variable
    with pytest.raises(ValueError, match="add_lmi_coo"):
        k.add_lmi_coo(4, [0, 1, 3], [0, 1], [0, 1], [1.0, 1.0])  # ptr points past row


def test_a_host_only_context_accepts_and_counts_the_constraint():
    k = KktContext(3, device=-1)
    # A_0 = e_0 e_0', A_1 empty, A_2 with an explicit zero and an off-diagonal entry, C = 2 I; entries in any order
    ptr, row, col, val = [0, 1, 1, 3, 7], [0, 3, 2, 3, 0, 2, 1], [0, 1, 2, 3, 0, 2, 1], [1.0, 0.5, 0.0, 2.0, 2.0, 2.0, 2.0]
    assert k.add_lmi_coo(4, ptr, row, col, val) == 0
    assert k.add_lmi_coo(4, ptr[:1] + [p for p in ptr[2:]], row, col, val, [2, 0]) == 1  # two variables of three
    assert k.cons == [("lmi", 4, 3), ("lmi", 4, 2)]
    assert k.count_sparse_affine() == -1 and k.count_sparse_lmi() == -1  # nothing is chosen before initialize
    k.initialize()
    assert k.N == 3 and k.L.cxk_num_constraints(k.h) == 2
    assert k.L.cxk_dual_size(k.h, 0) == 16
    assert k.count_sparse_lmi() == 0 and k.count_sparse_affine() == 0  # a host-only context chooses no kernels


def test_finalize_refuses_the_constraint_when_the_sparse_route_is_off(monkeypatch):
    monkeypatch.setenv("CXK_SPARSE_LMI", "0")
    k = host_context()
    assert k.add_lmi_coo(4, [0, 1, 2], [0, 1], [0, 1], [1.0, 1.0]) == 0
    assert k.L.cxk_finalize(k.h) != 0
    assert k.L.cxk_last_error(k.h).decode() == ec.R_FINALIZE
    monkeypatch.setenv("CXK_SPARSE_LMI", "1")
    assert k.L.cxk_finalize(k.h) == 0


def test_the_mode_setter_checks_its_argument_and_the_context_state():
    k = host_context()
    for mode in (-2, 2):
        with pytest.raises(KktError, match=r"cxk_set_sparse_affine.*mode"):
            k.set_sparse_affine(mode)
    for ok in (-1, 0, 1):
        k.set_sparse_affine(ok)
    assert k.add_lmi_coo(4, [0, 1, 2], [0, 1], [0, 1], [1.0, 1.0]) == 0
    k.initialize()
    with pytest.raises(KktError, match=r"cxk_set_sparse_affine.*finalized"):
        k.set_sparse_affine(1)


def test_the_prototypes_exist_in_the_library_and_in_capi():
    L = load_library()
    for name in ("cxk_add_lmi_coo", "cxk_set_sparse_affine", "cxk_count_sparse_affine"):
        assert getattr(L, name).argtypes is not None
    A = ca.api()
    for name in ("CONEX_HIP_AddLMIConstraintFromEntries", "CONEX_HIP_SetSparseAffine", "CONEX_HIP_CountSparseAffine"):
        assert getattr(A, name).argtypes is not None
    p = A.CONEX_CreateConeProgram()
    assert all(A.CONEX_HIP_SetSparseAffine(p, mode) == 0 for mode in (1, -1, 0))
    assert A.CONEX_HIP_SetSparseAffine(p, 2) != 0 and A.CONEX_HIP_SetSparseAffine(p, -2) != 0
    assert A.CONEX_HIP_CountSparseAffine(p) == -1  # no device context before a first solve
    A.CONEX_DeleteConeProgram(p)


# ------------------------------------------------------------------------------------ the route, compiled alone
SRC = r'''
#include "cone_route.h"
using namespace cxk_host;
extern "C" int lmi_route(int n, int m, int csr_only, int sparse_lmi, int sparse_pays, int symmetric, const char** refusal) {
  ConeShape s;
  s.type = CXK_LMI; s.n = n; s.m = m; s.csr_only = csr_only != 0; s.sparse_pays = sparse_pays != 0; s.symmetric = symmetric != 0;
  RouteModes md;
  md.sparse_lmi = sparse_lmi;
  const RouteChoice c = Choose(s, md);
  *refusal = c.refusal;
  return c.refusal ? -1 : c.route == ConeRoute::kLmiSparse ? 1 : c.route == ConeRoute::kLmiDense ? 0 : 2;
}
extern "C" int affine_pays(double n, double nnz_c, double npos) { return LmiSparseAffinePays(n, nnz_c, npos); }
extern "C" int affine_pays_at(double n, double nnz_c, double npos, double ratio) { return LmiSparseAffinePays(n, nnz_c, npos, ratio); }
extern "C" void affine_defaults(double* out) {
  const RouteModes m;
  out[0] = kSparseAffineMinRatio; out[1] = kSparseAffineMinNnz; out[2] = kSparseLmiMaxIndex; out[3] = m.sparse_affine;
  out[4] = m.sparse_affine_min_ratio;
}
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("lmi_entries_route")
    src = d / "lmi_entries_route_test.cc"
    src.write_text(SRC)
    so = d / "liblmi_entries_route_test.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "conex_amd", "csrc"), str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    L.lmi_route.restype = C.c_int
    L.lmi_route.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_char_p)]
    L.affine_pays.restype = C.c_int
    L.affine_pays.argtypes = [C.c_double] * 3
    L.affine_pays_at.restype = C.c_int
    L.affine_pays_at.argtypes = [C.c_double] * 4
    L.affine_defaults.restype = None
    L.affine_defaults.argtypes = [C.POINTER(C.c_double)]
    return L


def route(lib, n, m, csr_only, sparse_lmi, sparse_pays=False, symmetric=True):
    why = C.c_char_p()
    r = lib.lmi_route(n, m, int(csr_only), sparse_lmi, int(sparse_pays), int(symmetric), C.byref(why))
    return why.value.decode() if r < 0 else ("dense", "sparse", "other")[r]


# (n, m, csr_only, CXK_SPARSE_LMI, sparse_pays) -> route or refusal
ROUTE_TABLE = [
    ((9, 3, True, -1, False), "sparse"),       # whatever LmiSparsePays says
    ((9, 3, True, -1, True), "sparse"),
    ((9, 3, True, 1, False), "sparse"),
    ((4000, 4000, True, -1, False), "sparse"),
    ((9, 3, True, 0, True), ec.R_FINALIZE),
    ((4000, 4000, True, 0, False), ec.R_FINALIZE),
    ((9, 3, False, -1, False), "dense"),       # a constraint with dense matrices chooses as before
    ((9, 3, False, -1, True), "sparse"),
    ((9, 3, False, 0, True), "dense"),
    ((9, 3, False, 1, False), "sparse"),
]


@pytest.mark.parametrize("args,expected", ROUTE_TABLE)
def test_the_route_of_a_constraint_given_by_entries(lib, args, expected):
    assert route(lib, *args) == expected


def test_the_affine_threshold(lib):
    out = (C.c_double * 5)()
    lib.affine_defaults(out)
    ratio, min_nnz, max_index, mode, mode_ratio = list(out)
    assert (min_nnz, max_index, mode, mode_ratio) == (64, 32767, -2, ratio) and ratio > 0
    # R (nnz_c + npos) <= 4 n^2, and only with more than 64 nonzeros in C
    for n, nnz_c, npos in [(64, 65, 70), (500, 3400, 3900), (4000, 28000, 32000), (64, 4096, 4096), (130, 400, 16900),
                           (64, 64, 64), (1000, 64, 1000), (1000, 65, 1000)]:
        expect = nnz_c > 64 and ratio * (nnz_c + npos) <= 4.0 * n * n
        assert bool(lib.affine_pays(n, nnz_c, npos)) == expect, (n, nnz_c, npos)
    # the edges of the rule itself, at a ratio given here
    assert lib.affine_pays_at(100, 65, 4935, 8.0) == 1      # 8 * 5000 == 4 * 100^2
    assert lib.affine_pays_at(100, 65, 4936, 8.0) == 0
    assert lib.affine_pays_at(100, 64, 10, 8.0) == 0        # rides in the pair sums as list m
    assert lib.affine_pays_at(100, 65, 10, 0.0) == 1
    # max-cut, the family the entry point is for, moves at every order beyond LDS; a full C at a small order does not
    assert lib.affine_pays(4000, 28000, 32000) == 1 and lib.affine_pays(70, 4900, 4900) == 0


# ------------------------------------------------------------------------------------ the program layer
def test_the_python_class_builds_the_constraint_and_its_operator():
    e = syn.maxcut_entries(12)
    p = Conex(12)
    cid = p.AddLinearMatrixInequalityFromEntries(12, e["ptr"], e["row"], e["col"], e["val"])
    assert cid == 0 and p.num_constraints == 1
    d = syn.maxcut_problem(12)
    y = np.linspace(-1, 1, 12)
    assert np.array_equal(p.A[0].apply(y), np.einsum("i,ijk->jk", y, d["A"][0]))
    X = ec.symmetric_w(12)
    assert np.allclose(p.A[0].adjoint(X), np.einsum("ijk,jk->i", d["A"][0], X), rtol=1e-15, atol=0)
    assert np.array_equal(p.c[0], d["C"][0])
    p.SetSparseAffine(1)
    with pytest.raises(ConexError):
        p.SetSparseAffine(3)
    # the update calls fail on such a constraint
    with pytest.raises(ConexError):
        p.UpdateLinearOperator(cid, 1.0, 0, 1, 1)
    with pytest.raises(ConexError):
        p.UpdateAffineTerm(cid, 1.0, 1, 1)
    A = ca.api()
    assert A.CONEX_UpdateLinearOperator(p.a, cid, 1.0, 0, 1, 1, 0) != 0
    assert A.CONEX_UpdateAffineTerm(p.a, cid, 1.0, 1, 1, 0) != 0


@pytest.mark.parametrize("bad", ["ptr_short", "row_below_col", "index", "nan", "ptr_decreases", "variables"])
def test_the_program_layer_refuses_bad_lists(bad):
    p = Conex(2)
    ptr, row, col, val, v = [0, 1, 2, 3], [0, 1, 1], [0, 1, 0], [1.0, 1.0, 0.5], None
    if bad == "ptr_short":
        ptr = [0, 1, 2]
    elif bad == "row_below_col":
        row, col = [0, 1, 0], [0, 1, 1]
    elif bad == "index":
        row = [0, 3, 1]
    elif bad == "nan":
        val = [1.0, float("nan"), 0.5]
    elif bad == "ptr_decreases":
        ptr = [0, 2, 1, 3]
    else:
        v, ptr = [0, 5], [0, 1, 2, 3]
    with pytest.raises(ConexError):
        p.AddLinearMatrixInequalityFromEntries(3, ptr, row, col, val, v)
    assert p.num_constraints == 0
    assert p.AddLinearMatrixInequalityFromEntries(3, [0, 1, 2, 3], [0, 1, 1], [0, 1, 0], [1.0, 1.0, 0.5]) == 0
