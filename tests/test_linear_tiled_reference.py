"""The rows of test_gpu_linear_tiled.py on the float64 oracle, and the host side of the switch.

The oracle takes a linear block of any shape, so every row of the tiled kernels' matrix runs through the GPU
file's whole comparison (km.run_rows) on it, at the three scaling points and under the same bounds: correct
float64 code meets them at these lengths, which is what lets the GPU test use the existing constants unchanged.
The worst quantity must use a visible part of its bound (the bounds are not slack) without passing it.
Nothing here needs a GPU.
"""
import functools

import pytest

import conex_api as ca
import oracle_lib as ol
import test_gpu_cone_kernel_matrix as km
import test_gpu_linear_tiled as lt
from conex_amd import KktContext
from conex_amd.kkt import KktError, load_library


@functools.lru_cache(maxsize=None)
def oracle_report(row_id, point):
    row = lt.ROWS[lt.ROW_IDS.index(row_id)]
    cones, cliques, num_vars = km.make_problem(row, point, lt.row_seed(row))
    return tuple(km.run_rows(ol.Program, cones, cliques, num_vars, lt.row_seed(row) + 1, [],
                             short_step=row_id in lt.SHORT_STEP_ROWS))


@pytest.mark.parametrize("point", km.POINTS, ids=lt.POINT_IDS)
@pytest.mark.parametrize("row", lt.ROWS, ids=lt.ROW_IDS)
def test_the_float64_oracle_meets_the_bounds_on_the_tiled_rows(row, point):
    assert oracle_report(row[0], point)


def test_the_bounds_are_neither_empty_nor_slack():
    worst = max(w for row in lt.ROWS for point in km.POINTS for _, w in oracle_report(row[0], point))
    assert 1e-3 <= worst <= 1.0, worst


@pytest.mark.parametrize("point", km.POINTS, ids=lt.POINT_IDS)
def test_the_float64_oracle_meets_the_bounds_on_the_widest_block(point):
    cn, cliques, m, y = lt.widest_case(point)
    o = km.build(ol.Program, [cn], cliques, m)
    km.set_points(o, [cn])
    report = lt.check_widest(o, cn, y, [])
    assert len(report) == 6 and max(w for _, w in report) <= 1.0


def test_the_rows_sit_on_their_edges():
    lt.test_rows_sit_on_their_edges()


def test_the_wide_line_search_case_meets_its_precondition():
    *_, want, _ = lt.wide_line_search_expected()
    assert want > 0


# ------------------------------------------------------------------------------------ the switch, host side
def host_context():
    k = KktContext(10, device=-1)
    return k


def add_block(k):
    import numpy as np
    assert k.add_linear(np.full((20, 10), 0.01), np.ones(20)) == 0


def test_a_host_only_context_counts_no_tiled_blocks():
    k = host_context()
    k.set_tiled_linear(1)
    add_block(k)
    assert k.count_tiled_linear() == -1  # nothing is chosen before initialize
    k.initialize()
    assert k.N == 10
    assert k.count_tiled_linear() == 0   # a host-only context chooses no kernels


def test_the_switch_is_refused_after_initialize_with_a_message():
    k = host_context()
    add_block(k)
    k.initialize()
    for mode in (1, 0, -1):
        with pytest.raises(KktError, match=r"cxk_set_tiled_linear.*finalized"):
            k.set_tiled_linear(mode)


@pytest.mark.parametrize("mode", [-2, 2])
def test_an_invalid_mode_is_refused(mode):
    k = host_context()
    with pytest.raises(KktError, match=r"cxk_set_tiled_linear.*mode"):
        k.set_tiled_linear(mode)
    for ok in (-1, 0, 1):
        k.set_tiled_linear(ok)


def test_the_prototypes_exist_in_the_library_and_in_capi():
    L = load_library()
    assert L.cxk_set_tiled_linear.argtypes is not None and L.cxk_count_tiled_linear.argtypes is not None
    A = ca.api()
    assert A.CONEX_HIP_SetTiledLinear.argtypes is not None
    p = A.CONEX_CreateConeProgram()
    assert A.CONEX_HIP_SetTiledLinear(p, 1) == 0 and A.CONEX_HIP_SetTiledLinear(p, -1) == 0
    assert A.CONEX_HIP_SetTiledLinear(p, 2) != 0
    A.CONEX_DeleteConeProgram(p)
