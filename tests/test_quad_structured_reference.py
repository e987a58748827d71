"""The rows of test_gpu_quad_structured.py on the float64 oracle, the operator-form reference against
cone_reference.quad_schur, and the host side of cxk_add_quadratic_structured.  Nothing here needs a GPU.

The oracle (ol.Program, dense add_quadratic) gets Q expanded in longdouble and rounded to float64: honest float64 work
on a Q perturbed by u |Q| stays inside the bounds of km.run_rows against the longdouble reference, which is what lets
the GPU test use the constants C_SCHUR, C_PREPARE, C_TAKE unchanged.  (The `segments` row, n = 4096, takes the oracle's
naive loops and the longdouble reference about ten seconds per scaling point; every other row well under one.)
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import cone_reference as ref
import oracle_lib as ol
import quad_structured_cases as qc
import test_gpu_cone_kernel_matrix as km
import test_gpu_quad_structured as gq
from conex_amd import KktContext
from conex_amd.kkt import KktError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINT_IDS = [p if isinstance(p, str) else f"cond{p:.0e}" for p in km.POINTS]
U_LD = 2.0 ** -64  # unit roundoff of the longdouble reference


@functools.lru_cache(maxsize=None)
def oracle_report(row_id, point):
    row = qc.ROWS[qc.ROW_IDS.index(row_id)]
    cones, cliques, num_vars = qc.make_problem(row, point)
    return km.run_rows(ol.Program, cones, cliques, num_vars, qc.row_seed(row) + 1, [], short_step=row_id in qc.SHORT_STEP_ROWS)


@pytest.mark.parametrize("point", km.POINTS, ids=POINT_IDS)
@pytest.mark.parametrize("row", qc.ROWS, ids=qc.ROW_IDS)
def test_the_float64_oracle_meets_the_bounds_on_the_structured_rows(row, point):
    assert oracle_report(row[0], point)


def test_the_rows_sit_on_their_edges():
    qc.test_rows_sit_on_their_edges()


# ------------------------------------------------------------------------------------ the restated reference
@pytest.mark.parametrize("row", [r for r in qc.ROWS if r[2] <= 300], ids=[r[0] for r in qc.ROWS if r[2] <= 300])
def test_the_operator_form_reference_equals_quad_schur_with_the_expanded_q(row):
    """To longdouble rounding, 64 u_ld x magnitude: this pins the restated formulas the n = 50 000 test leans on."""
    cones, _, _ = qc.make_problem(row, 1e6)
    for cn in cones:
        a = ref.quad_schur(cn["A"], cn["c"], cn["W"], cn["Q"])
        b = qc.quad_schur_op(cn["A"], cn["c"], cn["W"], cn["parts"])
        for key in ("G", "AW", "AQc", "sc"):
            (va, ma), (vb, mb) = a[key], b[key]
            assert np.all(np.abs(va - vb) <= 64 * U_LD * ma), key
            assert np.all(np.abs(ma - mb) <= 64 * U_LD * ma), key  # nonnegative parts: |Q| is the sum of the parts' |.|


def test_the_operators_equal_the_expansion():
    row = qc.ROWS[qc.ROW_IDS.index("duplicates")]
    cones, _, _ = qc.make_problem(row, "well")
    cn = cones[0]
    X = np.random.default_rng(1).uniform(-1, 1, (row[2], 3))
    Q = ref.ld(cn["Q"])
    assert np.all(np.abs(qc.apply_q(cn["parts"], X) - Q @ ref.ld(X)) <= 64 * U_LD * (np.abs(Q) @ np.abs(X)))
    assert np.all(np.abs(qc.apply_abs_q(cn["parts"], X[:, 0]) - np.abs(Q) @ ref.ld(X[:, 0])) <= 64 * U_LD * (np.abs(Q) @ np.abs(X[:, 0])))
    # the duplicates add up to the tridiagonal matrix they halve
    S_only = ref.ld(qc.expand(dict(cn["parts"], F=None, sigma=None), row[2]))
    ptr, idx, val = cn["parts"]["S"]
    assert np.array_equal(np.diag(S_only), ref.ld(2 * val[ptr[:-1] + 2 * np.minimum(np.arange(row[2]), 1)]))


# ------------------------------------------------------------------------------------ the host side
def host_pair(row_id):
    """The same A and vars through add_quadratic_structured and through add_quadratic, on host-only contexts."""
    row = qc.ROWS[qc.ROW_IDS.index(row_id)]
    cones, cliques, num_vars = qc.make_problem(row, "well")
    s, d = qc.StructuredQuad(num_vars, device=-1), KktContext(num_vars, device=-1)
    for i, (cn, cl) in enumerate(zip(cones, cliques)):
        assert s.add_quadratic(cn["Q"], cn["A"], cn["c"], cl) == i
        assert d.add_quadratic(np.asarray(cn["Q"], dtype=np.float64), cn["A"], cn["c"], cl) == i
    return s, d


@pytest.mark.parametrize("row_id", ["group-of-3", "m65", "chol"])
def test_a_host_only_context_takes_the_call_and_has_the_structure_of_add_quadratic(row_id):
    s, d = host_pair(row_id)
    assert s.count_structured_quadratic() == -1  # nothing before initialize
    s.initialize()
    d.initialize()
    assert s.N == d.N and list(s.order()) == list(d.order())
    assert s.count_structured_quadratic() == 0 and s.count_streamed_quadratic() == 0  # a host-only context chooses no kernels


def test_every_refusal_on_a_host_only_context():
    gq.check_refusals(-1)


def test_the_python_layer_checks_the_shapes_of_the_parts():
    k = KktContext(2, device=-1)
    A, c = np.full((5, 2), 0.01), np.r_[1.0, np.zeros(4)]
    ptr, idx, val = np.arange(5), np.arange(4), np.ones(4)
    with pytest.raises(ValueError, match="indptr has n \\+ 1 entries"):
        k.add_quadratic_structured((ptr[:-1], idx, val), None, None, A, c)
    with pytest.raises(ValueError, match="indptr has n \\+ 1 entries"):
        k.add_quadratic_structured((ptr, idx, val[:-1]), None, None, A, c)
    with pytest.raises(ValueError, match="F is \\(n, r\\)"):
        k.add_quadratic_structured(None, np.ones((3, 1)), None, A, c)
    with pytest.raises(ValueError, match="sigma has one entry per column"):
        k.add_quadratic_structured(None, np.ones((4, 2)), np.ones(3), A, c)
    with pytest.raises(ValueError, match="integers"):
        k.add_quadratic_structured((ptr.astype(float), idx, val), None, None, A, c)
    assert k.add_quadratic_structured((ptr, idx, val), None, None, A, c) == 0


# ------------------------------------------------------------------------------------ cone_route.h's pure functions
SRC = r'''
#include "cone_route.h"
using namespace cxk_host;
extern "C" int quad_csr_lanes(double nnz, double rows) { return QuadCsrLanes(nnz, rows); }
extern "C" int quad_factor_segments(int n, long long columns) { return QuadFactorSegments(n, columns); }
// type CXK_QUAD, structured: the route (7 = streamed, as tests/test_cone_route.py numbers it) or the refusal
extern "C" int quad_structured_choose(int n, int m, double nnz, int rank, int streamed_mode, const char** refusal) {
  ConeShape s;
  s.type = CXK_QUAD; s.n = n; s.m = m; s.has_q = true; s.q_structured = true; s.q_nnz = nnz; s.q_rank = rank;
  RouteModes md;
  md.streamed_quadratic = streamed_mode;
  const RouteChoice c = Choose(s, md);
  *refusal = c.refusal;
  return c.refusal ? -1 : c.route == ConeRoute::kQuadStreamed ? 7 : 0;
}
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("quad_structured_route")
    src = d / "quad_structured_route_test.cc"
    src.write_text(SRC)
    so = d / "libquad_structured_route_test.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "conex_amd", "csrc"), str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    L.quad_csr_lanes.restype = C.c_int
    L.quad_csr_lanes.argtypes = [C.c_double, C.c_double]
    L.quad_factor_segments.restype = C.c_int
    L.quad_factor_segments.argtypes = [C.c_int, C.c_longlong]
    L.quad_structured_choose.restype = C.c_int
    L.quad_structured_choose.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_char_p)]
    return L


def test_the_lanes_rule_and_the_segment_count_are_the_restated_ones(lib):
    for rows in (1, 7, 300, 16384):
        for mean in (0, 1, 3, 9, 26.9, 27, 27.1, 81, 242.9, 243, 243.1, 5000):
            nnz = float(int(mean * rows))
            assert lib.quad_csr_lanes(nnz, float(rows)) == qc.csr_lanes(nnz, rows), (rows, mean)
    assert lib.quad_csr_lanes(0.0, 0.0) == 1
    for n in (1, 1023, 1024, 2047, 2048, 4096, 100_000, 1_000_000):
        for columns in (0, 1, 2, 8, 65, 511, 512, 513, 100_000):
            assert lib.quad_factor_segments(n, columns) == qc.factor_segments(n, columns), (n, columns)
    assert lib.quad_factor_segments(1_000_000, 1) == 512 and lib.quad_factor_segments(1_000_000, 8) == 64


def choose(lib, n, m, nnz, rank, mode):
    why = C.c_char_p()
    r = lib.quad_structured_choose(n, m, float(nnz), rank, mode, C.byref(why))
    return r if r >= 0 else why.value.decode()


def test_a_structured_cone_takes_the_streamed_route_under_every_mode_and_beyond_the_dense_form(lib):
    for mode in (-1, 0, 1):
        assert choose(lib, 5, 4, 13, 1, mode) == 7             # tiny: no LDS form all the same
        assert choose(lib, 50_000, 3, 150_000, 2, mode) == 7   # n^2 beyond the int range
        assert choose(lib, 1_000_000, 8, 3e6, 8, mode) == 7
    # the demands that stay
    assert "(dimension + 1) x variables entries exceed the int range" in choose(lib, 1_000_000, 3000, 3e6, 1, 1)
    assert "variables x variables Schur block exceeds the int range" in choose(lib, 10, 46341, 10, 1, 1)
    assert "more than 2^31 nonzeros" in choose(lib, 1_000_000, 8, 2.0 ** 31, 1, 1)
    assert choose(lib, 1_000_000, 8, 2.0 ** 31 - 1, 1, 1) == 7


# ------------------------------------------------------------------------------------ Conex
class CsrStandIn:
    """What a scipy CSR matrix shows of itself: the three attributes, nothing else."""

    def __init__(self, indptr, indices, data):
        self.indptr, self.indices, self.data = indptr, indices, data


def test_conex_add_structured_quadratic_constraint_checks_its_arguments():
    from conex_amd.program import Conex, ConexError
    n, m = 4, 2
    A, c = np.full((n + 1, m), 0.01), np.r_[1.0, np.zeros(n)]
    ptr, idx, val = np.arange(n + 1), np.arange(n), np.full(n, 2.0)
    F = np.full((n, 2), 0.5)
    prog = Conex(m)
    bad = [
        dict(S=None, F=None),                                     # both parts absent
        dict(S=(ptr[:-1], idx, val)),                             # indptr too short
        dict(S=(ptr, idx[:-1], val)),                             # indices and data of different length
        dict(S=(np.array([0, 2, 1, 3, 4]), idx, val)),            # indptr decreases
        dict(S=(ptr, np.array([0, 1, 2, n]), val)),               # a column outside [0, n)
        dict(S=(ptr, idx, np.array([2.0, np.nan, 2.0, 2.0]))),    # a value that is not finite
        dict(F=np.full((n + 1, 2), 0.5)),                         # F with the wrong number of rows
        dict(F=np.where(np.arange(2 * n).reshape(n, 2) == 3, np.inf, 0.5)),
        dict(sigma=np.ones(3)),                                   # sigma of the wrong length
        dict(sigma=np.array([1.0, np.nan])),
        dict(A=np.full((n + 2, m), 0.01)),                        # A and c disagree
        dict(variables=[0]),                                      # fewer variables than columns
        dict(variables=[0, 7]),                                   # a variable outside the program
        dict(S=object()),                                         # neither a triple nor the three attributes
    ]
    for change in bad:
        kw = dict(dict(S=(ptr, idx, val), F=F, sigma=np.ones(2), A=A, c=c, variables=None), **change)
        with pytest.raises(ConexError):
            prog.AddStructuredQuadraticConstraint(kw["S"], kw["F"], kw["sigma"], kw["A"], kw["c"], kw["variables"])
    assert prog.num_constraints == 0
    # a triple, a stand-in for a scipy CSR matrix, either part alone, sigma left out
    assert prog.AddStructuredQuadraticConstraint((ptr, idx, val), F, np.ones(2), A, c) == 0
    assert prog.AddStructuredQuadraticConstraint(CsrStandIn(ptr, idx, val), F, None, A, c) == 1
    assert prog.AddStructuredQuadraticConstraint(CsrStandIn(ptr.astype(np.int64), idx.astype(np.int64), val), None, None, A, c, [1, 0]) == 2
    assert prog.AddStructuredQuadraticConstraint(None, F, [1.0, -0.25], A, c) == 3
    assert prog.num_constraints == 4
