"""The rows of test_gpu_soc_sparse.py without a GPU, the accuracy argument for the sparse route's formula, and the host
side of its interface.

The sparse route evaluates G = 4 u u' + 2 det(w) A' J A (u = A' w, J = diag(-1, 1, .., 1)) where the other two routes
form the literal 2 WA' WA through w^{1/2}.  Two findings carry the GPU file's bounds:

- componentwise: FormulaOracle below is the float64 oracle with the Schur stage replaced by a plain float64 numpy
  evaluation of the route's expressions in the kernels' summation orders (a thread's strided chain, the wavefront's
  butterfly, the waves in order; a column of H over its rows ascending).  Every row of the GPU file runs through that
  file's whole comparison on it at the three scaling points: the Schur stage meets C_SCHUR with g = 1 against
  cone_reference.quad_schur(A, c, W, None), the step stages (the oracle's own second-order cone) their usual bounds,
  and the worst quantity uses a visible part of its bound without passing it;
- end to end: min t s.t. |A x - b| <= t with a sparse 400 x 60 A solved by the oracle once with the literal cone
  (add_soc) and once in the Q(w) form (add_quadratic with Q = None) takes the same number of iterations to the same y.

Nothing here needs a GPU.
"""
import functools

import numpy as np
import pytest

import conex_api as ca
import oracle_lib as ol
import test_gpu_cone_kernel_matrix as km
import test_gpu_soc_sparse as sp
import test_gpu_soc_sparse_solve as sol
from conex_amd import KktContext
from conex_amd.kkt import KktError, load_library

BLOCK = 256  # kSocSparseBlock


def wave_sum(v):
    """WaveSum over the last axis (64 lanes): the butterfly's pairs, as a tree."""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def block_sum(terms):
    """BlockSum of per-element terms: thread t's chain over t, t + 256, .., the wavefronts' sums, the waves in order."""
    pad = (-len(terms)) % BLOCK
    chains = np.add.reduce(np.r_[terms, np.zeros(pad)].reshape(-1, BLOCK), axis=0)  # (row after row: a chain per thread)
    total = 0.0
    for wsum in wave_sum(chains.reshape(BLOCK // 64, 64)):
        total += wsum
    return total


def column_dots(A, x):
    """soc_sparse_dots: per column, each lane's chain over every 64th entry in ascending row, then WaveSum."""
    out = np.zeros(A.shape[1])
    for j in range(A.shape[1]):
        r = np.flatnonzero(A[:, j])
        t = A[r, j] * x[r]
        pad = (-len(t)) % 64
        out[j] = wave_sum(np.add.reduce(np.r_[t, np.zeros(pad)].reshape(-1, 64), axis=0)) if len(t) else 0.0
    return out


def sparse_route_float64(A, c, w):
    """(G, AW, AQc, sc) as kernels_soc_sparse.hip.h forms them, in float64."""
    n1, m = A.shape
    J = np.ones(n1)
    J[0] = -1.0
    H = np.zeros((m, m))
    for r in range(n1):  # a column's rows ascending; zeros add nothing
        H += np.outer(A[r], J[r] * A[r])
    h = column_dots(A, J * c)
    z = block_sum(np.r_[0.0, c[1:] * c[1:]]) - c[0] * c[0]
    det = w[0] * w[0] - block_sum(np.r_[0.0, w[1:] * w[1:]])
    wc = block_sum(w * c)
    u = column_dots(A, w)
    G = (4 * u)[:, None] * u[None, :] + (2 * det) * H
    return G, 2 * u, 2 * ((2 * wc) * u + det * h), np.array([2 * wc, 2 * ((2 * wc) * wc + det * z)])


class FormulaOracle(ol.Program):
    """The float64 oracle with the second-order cones' Schur stage evaluated by sparse_route_float64."""

    def __init__(self, num_vars):
        super().__init__(num_vars)
        self.data, self.points = {}, {}

    def add_soc(self, A, c, vars_=None):
        r = super().add_soc(A, c, vars_)
        self.data[r] = (np.array(A, dtype=np.float64), np.array(c, dtype=np.float64).ravel())
        return r

    def set_W(self, i, w):
        self.points[i] = np.array(w, dtype=np.float64).ravel()
        super().set_W(i, w)

    def constraint_schur(self, i):
        if i not in self.data:
            return super().constraint_schur(i)
        return sparse_route_float64(*self.data[i], self.points[i])


@functools.lru_cache(maxsize=None)
def formula_report(row_id, point):
    row = sp.ROWS[sp.ROW_IDS.index(row_id)]
    cones, cliques, num_vars = sp.make_problem(row, point)
    return tuple(sp.run_rows(FormulaOracle, cones, cliques, num_vars, sp.row_seed(row) + 1, [],
                             short_step=row_id in sp.SHORT_STEP_ROWS))


@pytest.mark.parametrize("point", km.POINTS, ids=sp.POINT_IDS)
@pytest.mark.parametrize("row", sp.ROWS, ids=sp.ROW_IDS)
def test_the_formula_in_float64_meets_the_bounds_on_the_sparse_rows(row, point):
    assert formula_report(row[0], point)


def test_the_bounds_are_neither_empty_nor_slack():
    worst = max(w for row in sp.ROWS for point in km.POINTS for _, w in formula_report(row[0], point))
    assert 1e-3 <= worst <= 1.0, worst
    schur = max(w for row in sp.ROWS for point in km.POINTS for what, w in formula_report(row[0], point)
                if what.split()[0] in ("G", "AW", "AQc", "scalars"))
    assert 1e-3 <= schur <= 1.0, schur


def test_the_rows_sit_on_their_edges():
    sp.test_rows_sit_on_their_edges()


def test_the_float64_evaluation_from_the_nonzeros_agrees_with_the_one_by_rows():
    """formula_from_nonzeros (the GPU file's check of the shapes beyond the longdouble reference) against
    sparse_route_float64 on a row both can do: within twice the bound of each other."""
    row, cones, cliques, num_vars, y = sp.row_problem("group-of-3", 1e6)
    cn = cones[0]
    A = cn["A"]
    r, j = np.nonzero(A)
    u, um, det, detm, AW, AQc, sc = sp.formula_from_nonzeros(row[3], row[4], r, j, A[r, j], cn["c"], cn["W"])
    G, AW2, AQc2, sc2 = sparse_route_float64(A, cn["c"], cn["W"])
    bound = 2 * km.C_SCHUR * km.U
    for got, (val, mag) in ((AW2, AW), (AQc2, AQc), (sc2, sc)):
        assert np.all(np.abs(got - val) <= bound * mag)


# ------------------------------------------------------------------------------------ end to end
def test_the_literal_cone_and_the_q_of_w_form_solve_the_same_program_alike():
    """The oracle's second-order cone assembles 2 WA' WA, its quadratic cone with Q = None the expressions of the
    sparse route: on the sparse least-squares program the iteration counts are equal and y agrees to 1e-10 relative
    (2.2e-13 measured)."""
    (M1, c1), (M2, c2), cost = sol.cone_data()
    out = []
    for form in ("soc", "quad"):
        o = ol.Program(sol.UNKNOWNS + 1)
        for M, c in ((M1, c1), (M2, c2)):
            assert (o.add_soc(M, c) if form == "soc" else o.add_quadratic(None, M, c)) >= 0
        ok, y = o.solve(cost, ol.default_config())
        assert ok == 1
        out.append((o.num_iterations(), y))
    assert out[0][0] == out[1][0]
    diff = float(np.linalg.norm(out[0][1] - out[1][1]) / np.linalg.norm(out[0][1]))
    print(f"literal against Q(w): {out[0][0]} iterations, y differs by {diff:.3g} relative")
    assert diff <= 1e-10, diff


def test_the_oracle_still_achieves_the_recorded_distance_to_lstsq():
    A, b = sol.least_squares_data()
    x_ls = np.linalg.lstsq(A, b, rcond=None)[0]
    oko, yo, _ = sol.oracle_solve(ol.default_config())
    measured = sol.rel(yo[:sol.UNKNOWNS], x_ls)
    assert oko == 1 and 0.5 * sol.X_VS_LSTSQ_ORACLE <= measured <= 2 * sol.X_VS_LSTSQ_ORACLE, measured


# ------------------------------------------------------------------------------------ the interface, host side
def host_context():
    return KktContext(10, device=-1)


def add_cone(k):
    assert k.add_soc(np.full((20, 10), 0.01), np.r_[1.0, np.zeros(19)]) == 0


def test_a_host_only_context_counts_no_sparse_cones():
    k = host_context()
    k.set_sparse_soc(1)
    add_cone(k)
    assert k.add_soc_csr([0, 1, 3], [2, 9, 0], [1.0, -1.0, 0.5], [1.0, 0.0]) == 1
    assert k.count_sparse_soc() == -1  # nothing is chosen before initialize
    k.initialize()
    assert k.N == 10
    assert k.count_sparse_soc() == 0   # a host-only context chooses no kernels
    assert k.sparse_soc_setup_ms() == 0.0
    assert k.count_streamed_cones() == 0


def test_the_switch_is_refused_after_initialize_with_a_message():
    k = host_context()
    add_cone(k)
    k.initialize()
    for mode in (1, 0, -1):
        with pytest.raises(KktError, match=r"cxk_set_sparse_soc.*finalized"):
            k.set_sparse_soc(mode)


@pytest.mark.parametrize("mode", [-2, 2])
def test_an_invalid_mode_is_refused(mode):
    k = host_context()
    with pytest.raises(KktError, match=r"cxk_set_sparse_soc.*mode"):
        k.set_sparse_soc(mode)
    for ok in (-1, 0, 1):
        k.set_sparse_soc(ok)


@pytest.mark.parametrize("rowptr,col,val,c,message", sp.REFUSALS)
def test_add_soc_csr_refuses_bad_input_by_name(rowptr, col, val, c, message):
    sp.check_refusal(host_context(), rowptr, col, val, c, message)


def test_add_soc_csr_checks_its_sizes_and_the_python_arguments():
    k = host_context()
    r, err = sp.raw_add(k, 0, 10, [0, 1], [0], [1.0], [1.0])
    assert r == -1 and "cxk_add_soc_csr: n is at least 1" in err
    with pytest.raises(ValueError, match="add_soc_csr"):
        k.add_soc_csr([0, 1], [0], [1.0], [1.0, 0.0])           # rowptr too short for len(c) rows
    with pytest.raises(ValueError, match="add_soc_csr"):
        k.add_soc_csr([0, 1, 3], [0, 1], [1.0, 1.0], [1.0, 0.0])  # rowptr points past col
    assert k.add_soc_csr([0, 1, 2], [0, 1], [1.0, 1.0], [1.0, 0.0], [3, 4]) == 0  # two variables of ten
    assert k.cons[-1] == ("soc", 1, 2)


def test_the_linear_csr_entry_point_keeps_its_messages():
    """cxk_add_linear_csr shares its checks with cxk_add_soc_csr: each names itself."""
    import ctypes as C
    k = host_context()
    ip = lambda a: np.asarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))
    dp = lambda a: np.asarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    assert k.L.cxk_add_linear_csr(k.h, 2, 10, ip([0, 2, 1]), ip([0, 1, 2]), dp([1.0] * 3), dp([1.0, 1.0]), None) == -1
    assert k.L.cxk_last_error(k.h).decode() == "cxk_add_linear_csr: rowptr decreases"
    assert k.L.cxk_add_linear_csr(k.h, 0, 10, ip([0]), ip([0]), dp([1.0]), dp([1.0]), None) == -1
    assert k.L.cxk_last_error(k.h).decode() == "cxk_add_linear_csr: rows is at least 1 and m at least 0"


def test_the_prototypes_exist_in_the_library_and_in_capi():
    L = load_library()
    for name in ("cxk_set_sparse_soc", "cxk_count_sparse_soc", "cxk_add_soc_csr", "cxk_sparse_soc_setup_ms"):
        assert getattr(L, name).argtypes is not None
    A = ca.api()
    assert A.CONEX_HIP_SetSparseSoc.argtypes is not None and A.CONEX_HIP_CountSparseSoc.argtypes is not None
    p = A.CONEX_CreateConeProgram()
    assert A.CONEX_HIP_SetSparseSoc(p, 1) == 0 and A.CONEX_HIP_SetSparseSoc(p, -1) == 0
    assert A.CONEX_HIP_SetSparseSoc(p, 0) == 0
    assert A.CONEX_HIP_SetSparseSoc(p, 2) != 0 and A.CONEX_HIP_SetSparseSoc(p, -2) != 0
    assert A.CONEX_HIP_CountSparseSoc(p) == -1  # no device context before a first solve
    A.CONEX_DeleteConeProgram(p)
