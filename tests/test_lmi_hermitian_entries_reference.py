"""Hermitian matrix inequalities given by their entries, host side (no GPU): the numpy model of the folded sums against
the dense formulas on the embedded matrices in longdouble; cxk_add_hermitian_coo's refusals, by their exact messages,
on a host-only context; the fold switch; the program layer."""
import ctypes as C

import numpy as np
import pytest

import lmi_hermitian_entries_cases as hc
from conex_amd import KktContext, capi as ca
from conex_amd import synthetic as syn
from conex_amd.kkt import KktError, load_library
from conex_amd.program import Conex, ConexError


# ------------------------------------------------------------------------------------ the model
def compare(case, W, bar):
    ref, got = hc.dense_formulas(case, W), hc.folded_model(case, W)
    for key in ("G", "AW", "AQc"):
        assert hc.rel(got[key], ref[key]) <= bar, key
    assert abs(got["cq"] - ref["cq"]) <= bar * abs(ref["cq"]) and abs(got["wc"] - ref["wc"]) <= bar * abs(ref["wc"])
    return got


@pytest.mark.parametrize("n,d,m", hc.MODEL_SHAPES)
def test_folded_sums_equal_the_dense_formulas(n, d, m):
    """The sums over the top block row, undivided, give tr(.) / d of the embedded matrices within 1e-14 of longdouble
    (a scratch run gave 6e-16); the top lists hold exactly 1 / d of the entries."""
    case = hc.make_case(n, d, m, per=3)
    got = compare(case, hc.hermitian_exponential(n, d), 1e-14)
    assert got["top"] * d == got["all"] and got["top"] > 0


@pytest.mark.parametrize("n,d,m", hc.MODEL_SHAPES)
def test_the_fold_is_stable_for_a_w_slightly_off_the_real_representations(n, d, m):
    """W as a step kernel leaves it: a real representation up to rounding.  The fold does not amplify that."""
    case = hc.make_case(n, d, m, per=3)
    W = hc.hermitian_exponential(n, d)
    W = W + 1e-16 * np.max(np.abs(W)) * np.random.default_rng(9).uniform(-1, 1, W.shape)
    assert not np.array_equal(W[:n, :n], W[n:2 * n, n:2 * n])  # (the diagonal blocks of a real representation are equal)
    compare(case, W, 1e-14)


def test_the_embedding_of_the_lists_is_the_embedding_of_the_planes():
    for d in (1, 2, 4):
        case = hc.make_case(7, d, 3, per=4, c="full")
        for i in range(4):
            R, C_, V = hc.embedded_list(case, i)
            M = np.zeros((7 * d, 7 * d))
            M[R, C_] = V
            want = hc.embed_planes(case["A"][i] if i < 3 else case["C"])
            assert np.array_equal(M, want) and np.array_equal(M, M.T) and len(V) == np.count_nonzero(want)
            r, c_, v, top = hc.folded_order(case, i)
            assert top * d == len(v) and np.all(r[:top] < 7) and np.all(r[top:] >= 7)


def test_the_generator_of_the_line_family():
    for d, n, m in ((2, 12, 12), (4, 9, 5), (1, 6, 6)):
        e = syn.hermitian_entries(n, d, m)
        assert e["val"].shape == (len(e["row"]), d) and np.all(e["row"] >= e["col"]) and len(e["ptr"]) == m + 2
        assert np.array_equal(e["C"][0], np.eye(n)) and not e["C"][1:].any()
        for i in range(m):
            s = slice(e["ptr"][i], e["ptr"][i + 1])
            assert 3 <= s.stop - s.start <= 4 and np.sum(e["row"][s] != e["col"][s]) == 1
            assert np.array_equal(e["A"][i, 0], e["A"][i, 0].T) and all(np.array_equal(p, -p.T) for p in e["A"][i, 1:])
            assert e["b"][i] == pytest.approx(0.5 * np.trace(e["A"][i, 0]))
    assert syn.hermitian_entries(100, 2, 5)["A"] is None
    r = syn.hermitian_entries(10, 4, 3, per_matrix=6)
    assert all(r["ptr"][i + 1] - r["ptr"][i] == 6 for i in range(3))


# ------------------------------------------------------------------------------------ the interface, host side
def raw_add(k, n, d, m, ptr, row, col, val, null=()):
    ip = lambda a: np.asarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))
    dp = lambda a: np.asarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    args = dict(ptr=ip(ptr), row=ip(row) if len(row) else ip([0]), col=ip(col) if len(col) else ip([0]),
                val=dp(val) if len(val) else dp([0.0]))
    for name in null:
        args[name] = None
    r = k.L.cxk_add_hermitian_coo(k.h, n, d, m, args["ptr"], args["row"], args["col"], args["val"], None)
    return r, k.L.cxk_last_error(k.h).decode()


@pytest.mark.parametrize("n,d,m,ptr,row,col,val,message", hc.REFUSALS)
def test_add_hermitian_coo_refuses_bad_input_by_name(n, d, m, ptr, row, col, val, message):
    k = KktContext(1, device=-1)
    r, err = raw_add(k, n, d, m, ptr, row, col, val)
    assert r == -1 and err == "cxk_add_hermitian_coo: " + message
    assert k.L.cxk_num_constraints(k.h) == 0


def test_add_hermitian_coo_refuses_null_pointers_too_many_variables_and_bad_shapes():
    k = KktContext(1, device=-1)
    good = (4, 2, 1, [0, 1, 2], [0, 1], [0, 1], [1.0, 0.0, 1.0, 0.0])
    assert raw_add(k, *good, null=("ptr",)) == (-1, "cxk_add_hermitian_coo: ptr is null")
    for name in ("row", "col", "val"):
        assert raw_add(k, *good, null=(name,)) == (-1, "cxk_add_hermitian_coo: row, col or val is null")
    assert raw_add(k, 4, 2, 32768, [0], [], [], []) == (-1, "cxk_add_hermitian_coo: " + hc.R_PACK)
    assert k.L.cxk_num_constraints(k.h) == 0
    with pytest.raises(ValueError, match="add_hermitian_coo"):
        k.add_hermitian_coo(4, 2, [0, 1], [0], [0], [[1.0, 0.0]])                      # ptr too short for one variable
    with pytest.raises(ValueError, match="add_hermitian_coo"):
        k.add_hermitian_coo(4, 2, [0, 1, 3], [0, 1], [0, 1], [[1.0, 0.0], [1.0, 0.0]])  # ptr points past row
    with pytest.raises(ValueError, match="add_hermitian_coo"):
        k.add_hermitian_coo(4, 2, [0, 1, 2], [0, 1], [0, 1], [1.0, 1.0])               # one plane per entry for d = 2
    with pytest.raises(ValueError, match="add_hermitian_coo"):
        k.add_hermitian_coo(4, 4, [0, 1, 2], [0, 1], [0, 1], np.array([1.0 + 0j, 1.0]))  # complex values are for d = 2


def test_a_host_only_context_accepts_and_counts_the_constraint():
    k = KktContext(3, device=-1)
    # A_0 = e_0 e_0^*, A_1 empty, A_2 with an all-zero entry, a purely imaginary one and a real diagonal one, C = 2 I
    ptr, row, col = [0, 1, 1, 4, 8], [0, 3, 2, 3, 0, 2, 1, 3], [0, 1, 2, 3, 0, 2, 1, 3]
    val = np.array([1.0, 0.5j, 0.0, 2.0, 2.0, 2.0, 2.0, 2.0])
    assert k.add_hermitian_coo(4, 2, ptr, row, col, val) == 0
    planes = np.stack([val.real, val.imag], axis=1)
    assert k.add_hermitian_coo(4, 2, ptr[:1] + ptr[2:], row, col, planes, [2, 0]) == 1  # two variables of three
    assert k.add_hermitian_coo(4, 1, ptr, row, col, val.real + val.imag) == 2           # over R: one plane
    assert k.cons == [("herm", 4, 3, 2), ("herm", 4, 2, 2), ("herm", 4, 3, 1)]
    assert k.count_sparse_fold() == -1 and k.count_sparse_lmi() == -1  # nothing is chosen before initialize
    k.initialize()
    assert k.N == 3 and k.L.cxk_num_constraints(k.h) == 3
    assert [k.L.cxk_dual_size(k.h, i) for i in range(3)] == [2 * 16, 2 * 16, 16]
    assert k.count_sparse_lmi() == 0 and k.count_sparse_fold() == 0  # a host-only context chooses no kernels


def test_finalize_refuses_the_constraint_when_the_sparse_route_is_off(monkeypatch):
    monkeypatch.setenv("CXK_SPARSE_LMI", "0")
    k = KktContext(1, device=-1)
    assert k.add_hermitian_coo(4, 2, [0, 1, 2], [0, 1], [0, 1], [[1.0, 0.0], [1.0, 0.0]]) == 0
    assert k.L.cxk_finalize(k.h) != 0
    assert k.L.cxk_last_error(k.h).decode() == hc.R_FINALIZE
    monkeypatch.setenv("CXK_SPARSE_LMI", "1")
    assert k.L.cxk_finalize(k.h) == 0


def test_the_fold_setter_checks_its_argument_and_the_context_state():
    k = KktContext(1, device=-1)
    for mode in (-2, -1, 2):
        with pytest.raises(KktError, match=r"cxk_set_sparse_fold.*mode"):
            k.set_sparse_fold(mode)
    for ok in (0, 1):
        k.set_sparse_fold(ok)
    assert k.add_hermitian_coo(4, 2, [0, 1, 2], [0, 1], [0, 1], [[1.0, 0.0], [1.0, 0.0]]) == 0
    k.initialize()
    with pytest.raises(KktError, match=r"cxk_set_sparse_fold.*finalized"):
        k.set_sparse_fold(1)


def test_the_prototypes_exist_in_the_library_and_in_capi():
    L = load_library()
    for name in ("cxk_add_hermitian_coo", "cxk_set_sparse_fold", "cxk_count_sparse_fold"):
        assert getattr(L, name).argtypes is not None
    A = ca.api()
    for name in ("CONEX_HIP_AddHermitianConstraintFromEntries", "CONEX_HIP_SetSparseFold", "CONEX_HIP_CountSparseFold"):
        assert getattr(A, name).argtypes is not None
    p = A.CONEX_CreateConeProgram()
    assert all(A.CONEX_HIP_SetSparseFold(p, mode) == 0 for mode in (1, 0))
    assert A.CONEX_HIP_SetSparseFold(p, 2) != 0 and A.CONEX_HIP_SetSparseFold(p, -1) != 0
    assert A.CONEX_HIP_CountSparseFold(p) == -1  # no device context before a first solve
    A.CONEX_DeleteConeProgram(p)
    names = [L.cxk_lmi_kernel_name(L.cxk_lmi_kernel_count() + 2 + q).decode() for q in range(5)]
    assert names == [s + " folded" for s in ("lmi_schur_sparse small", "lmi_schur_sparse small dense-C", "lmi_schur_sparse hbm",
                                             "lmi_schur_sparse hbm dense-C", "lmi_schur_sparse hbm sparse-C")]
    assert L.cxk_lmi_kernel_name(L.cxk_lmi_kernel_count() + 7) is None


# ------------------------------------------------------------------------------------ the program layer
def test_the_program_layer_takes_the_lists_and_refuses_bad_ones():
    e = syn.hermitian_entries(6, 2, 4)
    p = Conex(4)
    assert p.AddHermitianMatrixInequalityFromEntries(6, 2, e["ptr"], e["row"], e["col"], e["val"]) == 0
    z = e["val"][:, 0] + 1j * e["val"][:, 1]
    assert p.AddHermitianMatrixInequalityFromEntries(6, 2, e["ptr"], e["row"], e["col"], z) == 1  # complex values
    s = e["ptr"][1]                                                                                # (without A_0)
    assert p.AddHermitianMatrixInequalityFromEntries(6, 2, e["ptr"][1:] - s, e["row"][s:], e["col"][s:], e["val"][s:], [3, 1, 0]) == 2
    with pytest.raises(ConexError):
        p.UpdateLinearOperator(0, 1.0, 0, 1, 1, 0)
    with pytest.raises(ConexError):
        p.UpdateAffineTerm(0, 1.0, 1, 1, 0)
    bad = dict(ptr=e["ptr"], row=e["row"], col=e["col"], val=e["val"], d=2, variables=None)
    off = int(np.flatnonzero(e["row"] != e["col"])[0])
    dia = int(np.flatnonzero(e["row"] == e["col"])[0])

    def changed(**kw):
        a = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in bad.items()}
        for key, (at, v) in kw.items():
            a[key][at] = v
        return a

    for a in (dict(bad, ptr=e["ptr"][:-1]),                                  # a short ptr
              changed(row=(off, e["col"][off]), col=(off, e["row"][off])),    # row < col
              changed(row=(dia, 6), col=(dia, 6)),                           # an index outside [0, n)
              changed(val=((off, 1), float("nan"))),                         # a plane that is not finite
              changed(val=((dia, 1), 0.5)),                                  # a complex diagonal
              dict(bad, d=3, val=np.zeros((len(e["row"]), 3))),              # no such algebra
              dict(bad, variables=[0, 1, 2, 9])):                            # a variable the program does not have
        with pytest.raises(ConexError):
            p.AddHermitianMatrixInequalityFromEntries(6, a["d"], a["ptr"], a["row"], a["col"], a["val"], a["variables"])
    for mode in (2, -1):
        with pytest.raises(ConexError):
            p.SetSparseFold(mode)
    p.SetSparseFold(0), p.SetSparseFold(1)
