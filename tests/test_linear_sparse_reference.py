"""The rows of test_gpu_linear_sparse.py on the float64 oracle, and the host side of the sparse route's interface.

The oracle takes a linear block of any pattern, so every row of the sparse kernels' matrix runs through the GPU
file's whole comparison (km.run_rows) on it, at the three scaling points and under the same bounds: correct float64
code meets them on these patterns, which is what lets the GPU test use the existing constants unchanged.  The worst
quantity must use a visible part of its bound (the bounds are not slack) without passing it.  Nothing here needs a GPU.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import conex_api as ca
import oracle_lib as ol
import test_gpu_cone_kernel_matrix as km
import test_gpu_linear_sparse as ls
from conex_amd import KktContext
from conex_amd.kkt import KktError, load_library


@functools.lru_cache(maxsize=None)
def oracle_report(row_id, point):
    row = ls.ROWS[ls.ROW_IDS.index(row_id)]
    cones, cliques, num_vars = ls.make_problem(row, point)
    return tuple(km.run_rows(ol.Program, cones, cliques, num_vars, ls.row_seed(row) + 1, [],
                             short_step=row_id in ls.SHORT_STEP_ROWS))


@pytest.mark.parametrize("point", km.POINTS, ids=ls.POINT_IDS)
@pytest.mark.parametrize("row", ls.ROWS, ids=ls.ROW_IDS)
def test_the_float64_oracle_meets_the_bounds_on_the_sparse_rows(row, point):
    assert oracle_report(row[0], point)


def test_the_bounds_are_neither_empty_nor_slack():
    worst = max(w for row in ls.ROWS for point in km.POINTS for _, w in oracle_report(row[0], point))
    assert 1e-3 <= worst <= 1.0, worst


def test_the_rows_sit_on_their_edges():
    ls.test_rows_sit_on_their_edges()


@pytest.mark.parametrize("r,m,bind", ls.LS_CASES)
def test_the_line_search_cases_meet_their_preconditions(r, m, bind):
    *_, want, _ = ls.line_search_expected(r, m, bind)
    assert want > 0


def test_the_csr_helper_reproduces_its_matrix():
    rng = np.random.default_rng(8)
    A = ls.make_pattern("holes", 9, 6, rng)
    rowptr, col, val = ls.csr_of(A, rng)
    B = np.zeros_like(A)
    for r in range(A.shape[0]):
        cols = col[rowptr[r]:rowptr[r + 1]]
        assert len(set(cols)) == len(cols)
        B[r, cols] = val[rowptr[r]:rowptr[r + 1]]
    assert np.array_equal(A, B) and val.count(0.0) == 3
    assert any(col[rowptr[r]:rowptr[r + 1]] != sorted(col[rowptr[r]:rowptr[r + 1]]) for r in range(A.shape[0]))


# ------------------------------------------------------------------------------------ the interface, host side
def host_context():
    return KktContext(10, device=-1)


def add_block(k):
    assert k.add_linear(np.full((20, 10), 0.01), np.ones(20)) == 0


def test_a_host_only_context_counts_no_sparse_blocks():
    k = host_context()
    k.set_sparse_linear(1)
    add_block(k)
    assert k.add_linear_csr([0, 1, 3], [2, 9, 0], [1.0, -1.0, 0.5], np.ones(2)) == 1
    assert k.count_sparse_linear() == -1  # nothing is chosen before initialize
    k.initialize()
    assert k.N == 10
    assert k.count_sparse_linear() == 0   # a host-only context chooses no kernels


def test_the_switch_is_refused_after_initialize_with_a_message():
    k = host_context()
    add_block(k)
    k.initialize()
    for mode in (1, 0, -1):
        with pytest.raises(KktError, match=r"cxk_set_sparse_linear.*finalized"):
            k.set_sparse_linear(mode)


@pytest.mark.parametrize("mode", [-2, 2])
def test_an_invalid_mode_is_refused(mode):
    k = host_context()
    with pytest.raises(KktError, match=r"cxk_set_sparse_linear.*mode"):
        k.set_sparse_linear(mode)
    for ok in (-1, 0, 1):
        k.set_sparse_linear(ok)


def raw_add(k, rows, m, rowptr, col, val, c):
    ip = lambda a: None if a is None else np.asarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))
    dp = lambda a: None if a is None else np.asarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    keep = [np.asarray(a) for a in (rowptr, col, val, c) if a is not None]  # noqa: F841
    r = k.L.cxk_add_linear_csr(k.h, rows, m, ip(rowptr), ip(col), dp(val), dp(c), None)
    return r, k.L.cxk_last_error(k.h).decode()


@pytest.mark.parametrize("rowptr,col,val,c,message", [
    ([1, 2, 3], [0, 1, 2], [1.0, 1.0, 1.0], [1.0, 1.0], r"rowptr\[0\] is not 0"),
    ([0, 2, 1], [0, 1, 2], [1.0, 1.0, 1.0], [1.0, 1.0], r"rowptr decreases"),
    ([0, 1, 2], [0, 10], [1.0, 1.0], [1.0, 1.0], r"outside \[0, m\)"),
    ([0, 1, 2], [0, -1], [1.0, 1.0], [1.0, 1.0], r"outside \[0, m\)"),
    ([0, 3, 3], [4, 2, 4], [1.0, 1.0, 1.0], [1.0, 1.0], r"names a column twice"),
    (None, [0, 1], [1.0, 1.0], [1.0, 1.0], r"null"),
    ([0, 1, 2], None, [1.0, 1.0], [1.0, 1.0], r"null"),
    ([0, 1, 2], [0, 1], None, [1.0, 1.0], r"null"),
    ([0, 1, 2], [0, 1], [1.0, 1.0], None, r"null"),
])
def test_add_linear_csr_refuses_bad_input_by_name(rowptr, col, val, c, message):
    import re
    k = host_context()
    r, err = raw_add(k, 2, 10, rowptr, col, val, c)
    assert r == -1 and re.search(r"cxk_add_linear_csr.*" + message, err), err
    assert k.add_linear_csr([0, 1, 2], [0, 1], [1.0, 1.0], [1.0, 1.0]) == 0  # the context is still usable


def test_the_prototypes_exist_in_the_library_and_in_capi():
    L = load_library()
    for name in ("cxk_set_sparse_linear", "cxk_count_sparse_linear", "cxk_add_linear_csr"):
        assert getattr(L, name).argtypes is not None
    A = ca.api()
    assert A.CONEX_HIP_SetSparseLinear.argtypes is not None
    p = A.CONEX_CreateConeProgram()
    assert A.CONEX_HIP_SetSparseLinear(p, 1) == 0 and A.CONEX_HIP_SetSparseLinear(p, -1) == 0
    assert A.CONEX_HIP_SetSparseLinear(p, 0) == 0
    assert A.CONEX_HIP_SetSparseLinear(p, 2) != 0
    A.CONEX_DeleteConeProgram(p)
