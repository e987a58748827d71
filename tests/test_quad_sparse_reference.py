"""The rows of test_gpu_quad_sparse.py on the float64 oracle, the reference restated for a CSR A against
cone_reference.quad_schur, and the host side of cxk_add_quadratic_csr.  Nothing here needs a GPU.

The oracle (ol.Program, dense add_quadratic) gets the dense A whose zeros are the pattern and Q expanded and rounded to
float64: honest float64 work stays inside the bounds of km.run_rows against the longdouble reference at these shapes,
which is what lets the GPU test use the constants C_SCHUR, C_PREPARE, C_TAKE unchanged.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import cone_reference as ref
import oracle_lib as ol
import quad_sparse_cases as qs
import quad_structured_cases as qc
import test_gpu_cone_kernel_matrix as km
from conex_amd import KktContext
from conex_amd.kkt import KktError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINT_IDS = [p if isinstance(p, str) else f"cond{p:.0e}" for p in km.POINTS]
U_LD = 2.0 ** -64  # unit roundoff of the longdouble reference


@functools.lru_cache(maxsize=None)
def oracle_report(row_id, point):
    row = qs.ROWS[qs.ROW_IDS.index(row_id)]
    cones, cliques, num_vars = qs.make_problem(row, point)
    return km.run_rows(ol.Program, cones, cliques, num_vars, qs.row_seed(row) + 1, [], short_step=row_id in qs.SHORT_STEP_ROWS)


@pytest.mark.parametrize("point", km.POINTS, ids=POINT_IDS)
@pytest.mark.parametrize("row", qs.ROWS, ids=qs.ROW_IDS)
def test_the_float64_oracle_meets_the_bounds_on_the_sparse_rows(row, point):
    assert oracle_report(row[0], point)


def test_the_rows_sit_on_their_edges():
    qs.test_rows_sit_on_their_edges()


# ------------------------------------------------------------------------------------ the restated reference
@pytest.mark.parametrize("row", qs.ROWS, ids=qs.ROW_IDS)
def test_the_reference_for_a_csr_a_equals_quad_schur_on_the_expanded_a(row):
    """To longdouble rounding, 64 u_ld x magnitude: this pins the restated formulas the n = 2^20 test leans on."""
    cones, _, _ = qs.make_problem(row, 1e6)
    for cn in cones:
        a = ref.quad_schur(cn["A"], cn["c"], cn["W"], cn["Q"])
        b = qs.quad_schur_op(qs.csr_of(cn["A"]), cn["m"], cn["c"], cn["W"], cn["Q"], cn["parts"])
        c = qs.quad_schur_op(qs.descending(qs.csr_of(cn["A"])), cn["m"], cn["c"], cn["W"], cn["Q"], cn["parts"])
        for key in ("G", "AW", "AQc", "sc"):
            (va, ma), (vb, mb), (vc, _) = a[key], b[key], c[key]
            assert np.all(np.abs(va - vb) <= 64 * U_LD * ma), key
            assert np.all(np.abs(ma - mb) <= 64 * U_LD * ma), key
            assert np.all(np.abs(va - vc) <= 64 * U_LD * ma), key


# ------------------------------------------------------------------------------------ the host side
def host_pair(row_id):
    """The same cones through add_quadratic_csr and through add_quadratic with the expanded A, on host-only contexts."""
    row = qs.ROWS[qs.ROW_IDS.index(row_id)]
    cones, cliques, num_vars = qs.make_problem(row, "well")
    s, d = qs.SparseAQuad(num_vars, device=-1), KktContext(num_vars, device=-1)
    for i, (cn, cl) in enumerate(zip(cones, cliques)):
        assert s.add_quadratic(cn["Q"], cn["A"], cn["c"], cl) == i
        assert d.add_quadratic(None if cn["Q"] is None else np.asarray(cn["Q"], dtype=np.float64), cn["A"], cn["c"], cl) == i
    return s, d


@pytest.mark.parametrize("row_id", ["group-of-3", "panel", "empty", "full-none"])
def test_a_host_only_context_takes_the_call_and_has_the_structure_of_add_quadratic(row_id):
    s, d = host_pair(row_id)
    assert s.count_sparse_quadratic() == -1  # nothing before initialize
    s.initialize()
    d.initialize()
    assert s.N == d.N and list(s.order()) == list(d.order())
    assert s.count_sparse_quadratic() == 0 and s.count_streamed_quadratic() == 0  # a host-only context chooses no kernels


def refusal_cases():
    """(name, keyword changes to a good call, the message): every refusal cxk_add_quadratic_csr makes of A and of the
    forms of Q; the refusals of the parts are cxk_add_quadratic_structured's, sampled."""
    n, m = 4, 3
    ptr = np.array([0, 1, 3, 4, 4, 6], dtype=np.int32)
    idx = np.array([2, 0, 1, 2, 0, 2], dtype=np.int32)
    val = np.array([1.0, 0.5, -0.5, 0.25, 2.0, -1.0])
    sp = (np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.full(n, 2.0))
    good = dict(Q=None, A=(ptr, idx, val))
    return n, m, good, [
        ("rowptr-start", dict(A=(ptr + 1, np.r_[idx, 0].astype(np.int32), np.r_[val, 1.0])), r"a_rowptr\[0\] is not 0"),
        ("rowptr-decreases", dict(A=(np.array([0, 3, 1, 4, 4, 6], dtype=np.int32), idx, val)), r"a_rowptr decreases"),
        ("column-high", dict(A=(ptr, np.array([2, 0, 1, m, 0, 2], dtype=np.int32), val)), r"a column is outside \[0, m\)"),
        ("column-negative", dict(A=(ptr, np.array([2, 0, -1, 2, 0, 2], dtype=np.int32), val)), r"a column is outside \[0, m\)"),
        ("column-twice", dict(A=(ptr, np.array([2, 1, 1, 2, 0, 2], dtype=np.int32), val)), r"a row names a column twice"),
        ("value-nan", dict(A=(ptr, idx, np.where(np.arange(6) == 2, np.nan, val))), r"a_val holds a value that is not finite"),
        ("value-inf", dict(A=(ptr, idx, np.where(np.arange(6) == 5, -np.inf, val))), r"a_val holds a value that is not finite"),
        ("dense-nan", dict(Q=np.where(np.eye(n) > 0, np.nan, 0.0)), r"Q holds a value that is not finite"),
        ("parts-rowptr", dict(Q=dict(S=(sp[0] + 1, np.arange(5, dtype=np.int32) % n, np.full(5, 2.0)))), r"q_rowptr\[0\] is not 0"),
        ("parts-column", dict(Q=dict(S=(sp[0], np.array([0, 1, 2, n], dtype=np.int32), sp[2]))), r"a column of the sparse part is outside \[0, n\)"),
        ("parts-value", dict(Q=dict(S=(sp[0], sp[1], np.array([2.0, np.inf, 2.0, 2.0])))), r"q_val holds a value that is not finite"),
        ("parts-F", dict(Q=dict(F=np.where(np.arange(8).reshape(n, 2) == 3, np.nan, 0.5))), r"F holds a value that is not finite"),
        ("parts-sigma", dict(Q=dict(F=np.full((n, 2), 0.5), sigma=np.array([1.0, np.inf]))), r"sigma holds a value that is not finite"),
    ]


def check_refusals(device):
    from conex_amd.kkt import _dp, _ip
    n, m, good, cases = refusal_cases()
    c = np.r_[1.0, np.zeros(n)]
    k = KktContext(m, device=device)
    for name, change, message in cases:
        kw = dict(good, **change)
        with pytest.raises(KktError, match=r"cxk_add_quadratic_csr: " + message):
            k.add_quadratic_csr(kw["Q"], kw["A"], c)
    # what the Python layer cannot say: null pointers, a dense Q together with parts, a negative rank
    ptr, idx, val = good["A"]
    Qd = np.eye(n).ravel()
    args = lambda **o: [o.get("Q"), o.get("qp"), o.get("qc"), o.get("qv"), o.get("rank", 0), o.get("F"), None,
                        o.get("ap", _ip(ptr)), _ip(idx), _dp(val), o.get("c", _dp(c)), None]
    sp = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.full(n, 2.0)
    for o, message in [(dict(ap=None), "a_rowptr or c is null"), (dict(c=None), "a_rowptr or c is null"),
                       (dict(Q=_dp(Qd), qp=_ip(sp[0]), qc=_ip(sp[1]), qv=_dp(sp[2])), "Q is given dense and by its parts: one form, or none for the identity"),
                       (dict(Q=_dp(Qd), rank=1, F=_dp(np.ones(n))), "Q is given dense and by its parts: one form, or none for the identity"),
                       (dict(rank=-1), "rank is negative"), (dict(rank=2), "F is null")]:
        assert k.L.cxk_add_quadratic_csr(k.h, n, m, *args(**o)) == -1
        assert k.L.cxk_last_error(k.h).decode() == "cxk_add_quadratic_csr: " + message
    # the context stays usable, with each form of Q
    assert k.add_quadratic_csr(None, good["A"], c) == 0
    assert k.add_quadratic_csr(2.0 * np.eye(n), good["A"], c) == 1
    assert k.add_quadratic_csr(dict(S=sp, F=np.full((n, 2), 0.5)), good["A"], c) == 2
    assert k.add_quadratic_csr((sp, None, None), good["A"], c) == 3
    k.initialize()
    return k


def test_every_refusal_on_a_host_only_context():
    check_refusals(-1)


class CsrStandIn:
    """What a scipy CSR matrix shows of itself: the three attributes (and a shape), nothing else."""

    def __init__(self, indptr, indices, data, shape=None):
        self.indptr, self.indices, self.data, self.shape = indptr, indices, data, shape


def test_the_python_layer_takes_a_triple_or_an_attribute_object_and_checks_shapes():
    n, m, good, _ = refusal_cases()
    ptr, idx, val = good["A"]
    c = np.r_[1.0, np.zeros(n)]
    k = KktContext(m, device=-1)
    assert k.add_quadratic_csr(None, (ptr, idx, val), c) == 0
    assert k.add_quadratic_csr(None, CsrStandIn(ptr.astype(np.int64), idx.astype(np.int64), val, (n + 1, m)), c) == 1
    assert k.add_quadratic_csr(None, (ptr.tolist(), idx.tolist(), val.tolist()), c, [2, 0, 1]) == 2
    with pytest.raises(ValueError, match="indptr has rows \\+ 1 entries"):
        k.add_quadratic_csr(None, (ptr[:-1], idx, val), c)
    with pytest.raises(ValueError, match="indptr has rows \\+ 1 entries"):
        k.add_quadratic_csr(None, (ptr, idx, val[:-1]), c)
    with pytest.raises(ValueError, match="integers"):
        k.add_quadratic_csr(None, (ptr.astype(float), idx, val), c)
    with pytest.raises(ValueError, match="A is \\(indptr, indices, data\\)"):
        k.add_quadratic_csr(None, object(), c)
    with pytest.raises(ValueError, match="Q is None, \\(n, n\\), or the parts"):
        k.add_quadratic_csr(np.eye(n + 1), (ptr, idx, val), c)
    with pytest.raises(ValueError, match="neither a sparse part nor factors"):
        k.add_quadratic_csr(dict(), (ptr, idx, val), c)
    k.initialize()
    assert k.N == m


def test_conex_add_sparse_quadratic_constraint_takes_each_form_and_checks_its_arguments():
    from conex_amd.program import Conex, ConexError
    n, m, good, cases = refusal_cases()
    ptr, idx, val = good["A"]
    c = np.r_[1.0, np.zeros(n)]
    sp = np.arange(n + 1), np.arange(n), np.full(n, 2.0)
    prog = Conex(m)
    for _, change, _ in cases:
        kw = dict(good, **change)
        with pytest.raises(ConexError):
            prog.AddSparseQuadraticConstraint(kw["Q"], kw["A"], c)
    for bad in (dict(A=(ptr[:-1], idx, val)), dict(A=object()), dict(Q=np.eye(n + 1)), dict(Q=dict()), dict(variables=[0]),
                dict(variables=[0, 1, 7]), dict(c=np.r_[1.0, np.zeros(n + 1)])):
        kw = dict(dict(good, c=c, variables=None), **bad)
        with pytest.raises(ConexError):
            prog.AddSparseQuadraticConstraint(kw["Q"], kw["A"], kw["c"], kw["variables"])
    assert prog.num_constraints == 0
    assert prog.AddSparseQuadraticConstraint(None, (ptr, idx, val), c) == 0
    assert prog.AddSparseQuadraticConstraint(2.0 * np.eye(n), CsrStandIn(ptr, idx, val, (n + 1, m)), c) == 1
    assert prog.AddSparseQuadraticConstraint(dict(S=CsrStandIn(*sp), F=np.full((n, 2), 0.5), sigma=[1.0, 0.5]), (ptr, idx, val), c, [2, 1, 0]) == 2
    assert prog.AddSparseQuadraticConstraint((None, np.full((n, 1), 0.5), None), qs.descending((ptr, idx, val)), c) == 3
    assert prog.num_constraints == 4


# ------------------------------------------------------------------------------------ cone_route.h's pure functions
SRC = r'''
#include "cone_route.h"
using namespace cxk_host;
extern "C" int quad_gram_panel_cols(int n, long long count) { return QuadGramPanelCols(n, count); }
// type CXK_QUAD added by its nonzeros: the route (7 = streamed, as tests/test_cone_route.py numbers it) or the refusal
extern "C" int quad_csr_choose(int n, int m, double nnz, int q_form, double q_nnz, int streamed_mode, int csr_only,
                               const char** refusal) {
  ConeShape s;
  s.type = CXK_QUAD; s.n = n; s.m = m; s.csr_only = csr_only != 0; s.nnz = nnz;
  s.has_q = q_form != 0; s.q_structured = q_form == 2; s.q_nnz = q_nnz; s.q_rank = q_form == 2 ? 1 : 0;
  RouteModes md;
  md.streamed_quadratic = streamed_mode;
  const RouteChoice c = Choose(s, md);
  *refusal = c.refusal;
  return c.refusal ? -1 : c.route == ConeRoute::kQuadStreamed ? 7 : c.route == ConeRoute::kQuadLds ? 6 : 0;
}
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("quad_sparse_route")
    src = d / "quad_sparse_route_test.cc"
    src.write_text(SRC)
    so = d / "libquad_sparse_route_test.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "conex_amd", "csrc"), str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    L.quad_gram_panel_cols.restype = C.c_int
    L.quad_gram_panel_cols.argtypes = [C.c_int, C.c_longlong]
    L.quad_csr_choose.restype = C.c_int
    L.quad_csr_choose.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_char_p)]
    return L


def test_the_panel_rule_is_the_restated_one(lib):
    for n in (1, 64, 1000, 4096, 2 ** 16, 2 ** 18, 2 ** 20, 2 ** 22, 2 ** 24, 2 ** 30):
        for count in (0, 1, 2, 3, 7, 100, 65536):
            assert lib.quad_gram_panel_cols(n, count) == qs.panel_cols(n, count), (n, count)
    assert lib.quad_gram_panel_cols(2 ** 20, 1) == 16 and lib.quad_gram_panel_cols(64, 2) == 64
    assert lib.quad_gram_panel_cols(2 ** 30, 65536) == 4  # never below four columns


def choose(lib, n, m, nnz, q_form, mode, q_nnz=0.0, csr_only=1):
    why = C.c_char_p()
    r = lib.quad_csr_choose(n, m, float(nnz), q_form, float(q_nnz), mode, csr_only, C.byref(why))
    return r if r >= 0 else why.value.decode()


IDENTITY, DENSE, PARTS = 0, 1, 2


def test_a_cone_added_by_its_nonzeros_takes_the_streamed_route_under_every_mode(lib):
    for mode in (-1, 0, 1):
        for form in (IDENTITY, DENSE, PARTS):
            assert choose(lib, 5, 4, 13, form, mode) == 7                    # tiny: no LDS form all the same
            assert choose(lib, 40, 41, 41, form, mode) == 7
        # (n + 1) m = 2^31 + 2048: refused with a dense A, taken by its nonzeros (a dense Q of that order has no room)
        assert choose(lib, 2 ** 20, 2048, 2 ** 20 + 2048, IDENTITY, mode) == 7
        assert choose(lib, 2 ** 20, 2048, 2 ** 20 + 2048, PARTS, mode, q_nnz=2 ** 20) == 7
        assert "(dimension + 1) x variables entries exceed the int range" in choose(lib, 2 ** 20, 2048, 0, PARTS, mode, 2 ** 20, csr_only=0)
    assert "(dimension + 1) x variables entries exceed the int range" in choose(lib, 2 ** 20, 2048, 0, IDENTITY, 1, csr_only=0)
    # the demands that stay
    for form in (IDENTITY, DENSE, PARTS):
        assert "variables x variables Schur block exceeds the int range" in choose(lib, 10, 46341, 10, form, 1)
        assert choose(lib, 10, 46340, 10, form, 1) == 7
    assert "inner-product matrix has more than 2^31 entries" in choose(lib, 46341, 3, 10, DENSE, 0)
    assert choose(lib, 46340, 3, 10, DENSE, 0) == 7 and choose(lib, 46341, 3, 10, PARTS, 0) == 7
    assert "sparse part has more than 2^31 nonzeros" in choose(lib, 10 ** 6, 8, 10, PARTS, 1, q_nnz=2.0 ** 31)
    # the new one, by name
    for form in (IDENTITY, DENSE, PARTS):
        assert choose(lib, 1000, 8, 2.0 ** 31 - 1, form, 1) == 7
        why = choose(lib, 1000, 8, 2.0 ** 31, form, 1)
        assert "added by cxk_add_quadratic_csr with more than 2^31 nonzeros" in why
    # a dense-A cone is chosen as before: the field does not leak
    assert choose(lib, 5, 4, 0, DENSE, 0, csr_only=0) == 6 and choose(lib, 5, 4, 2.0 ** 40, DENSE, 1, csr_only=0) == 7
