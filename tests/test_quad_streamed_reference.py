"""The rows of test_gpu_quad_streamed.py on the float64 oracle, and the host side of the switch.

The oracle takes a quadratic cone of any size, so every row of the streamed kernels' matrix runs through the GPU
file's whole comparison (km.run_rows) on it, at the three scaling points and under the same bounds: correct float64
code meets them at these sizes, which is what lets the GPU test use the existing constants unchanged.  Nothing here
needs a GPU.
"""
import functools

import pytest

import oracle_lib as ol
import test_gpu_cone_kernel_matrix as km
import test_gpu_quad_streamed as qs
from conex_amd import KktContext
from conex_amd.kkt import KktError

POINT_IDS = [p if isinstance(p, str) else f"cond{p:.0e}" for p in km.POINTS]


@functools.lru_cache(maxsize=None)
def oracle_report(row_id, point):
    row = qs.ROWS[qs.ROW_IDS.index(row_id)]
    cones, cliques, num_vars = km.make_problem(row, point, qs.row_seed(row))
    return km.run_rows(ol.Program, cones, cliques, num_vars, qs.row_seed(row) + 1, [], short_step=row_id in qs.SHORT_STEP_ROWS)


@pytest.mark.parametrize("point", km.POINTS, ids=POINT_IDS)
@pytest.mark.parametrize("row", qs.ROWS, ids=qs.ROW_IDS)
def test_the_float64_oracle_meets_the_bounds_on_the_streamed_rows(row, point):
    assert oracle_report(row[0], point)


def test_the_rows_sit_on_their_edges():
    qs.test_rows_sit_on_their_edges()


# ------------------------------------------------------------------------------------ the switch, host side
def host_context(mode=None):
    A, c = km.soc_data(5103, 4)
    k = KktContext(4, device=-1)
    if mode is not None:
        k.set_streamed_quadratic(mode)
    assert k.add_quadratic(None, A, c) == 0
    return k


@pytest.mark.parametrize("mode", [None, -1, 0, 1])
def test_a_host_only_context_runs_its_symbolic_analysis_whatever_the_mode(mode):
    k = host_context(mode)
    assert k.count_streamed_quadratic() == -1  # nothing is chosen before initialize
    k.initialize()
    assert k.N == 4 and list(k.order()) == [0]
    assert k.count_streamed_quadratic() == 0   # a host-only context chooses no kernels
    assert k.count_streamed_cones() == 0


def test_the_switch_is_refused_after_initialize_with_a_message():
    k = host_context()
    k.initialize()
    for mode in (-1, 0, 1):
        with pytest.raises(KktError, match=r"cxk_set_streamed_quadratic.*finalized"):
            k.set_streamed_quadratic(mode)


@pytest.mark.parametrize("mode", [-2, 2])
def test_a_mode_outside_the_three_is_refused_with_a_message(mode):
    k = host_context()
    with pytest.raises(KktError, match=r"cxk_set_streamed_quadratic.*mode"):
        k.set_streamed_quadratic(mode)
    k.set_streamed_quadratic(1)  # the context is still usable
    k.initialize()
