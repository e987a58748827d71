"""The rows of test_gpu_soc_streamed.py on the float64 oracle, and the host side of the switch.

The oracle takes a second-order cone of any size, so every row of the streamed kernels' matrix runs
through the GPU file's whole comparison (km.run_rows) on it, at the three scaling points and under the
same bounds: correct float64 code meets them at these lengths, which is what lets the GPU test use
the existing constants unchanged.  Nothing here needs a GPU.
"""
import functools

import numpy as np
import pytest

import oracle_lib as ol
import test_gpu_cone_kernel_matrix as km
import test_gpu_soc_streamed as st
from conex_amd import KktContext
from conex_amd.kkt import KktError

POINT_IDS = [p if isinstance(p, str) else f"cond{p:.0e}" for p in km.POINTS]


@functools.lru_cache(maxsize=None)
def oracle_report(row_id, point):
    row = st.ROWS[st.ROW_IDS.index(row_id)]
    cones, cliques, num_vars = km.make_problem(row, point, st.row_seed(row))
    return km.run_rows(ol.Program, cones, cliques, num_vars, st.row_seed(row) + 1, [], short_step=row_id in st.SHORT_STEP_ROWS)


@pytest.mark.parametrize("point", km.POINTS, ids=POINT_IDS)
@pytest.mark.parametrize("row", st.ROWS, ids=st.ROW_IDS)
def test_the_float64_oracle_meets_the_bounds_on_the_streamed_rows(row, point):
    assert oracle_report(row[0], point)


def test_the_rows_sit_on_their_edges():
    st.test_rows_sit_on_their_edges()


# ------------------------------------------------------------------------------------ the switch, host side
def host_context(switch):
    A, c = km.soc_data(319, 62)
    k = KktContext(62, device=-1)
    if switch:
        k.set_streamed_cones()
    assert k.add_soc(A, c) == 0
    return k


def test_a_host_only_context_still_runs_its_symbolic_analysis_with_the_switch_on():
    k = host_context(True)
    assert k.count_streamed_cones() == -1  # nothing is chosen before initialize
    k.initialize()
    assert k.N == 62 and list(k.order()) == [0]
    assert k.count_streamed_cones() == 0   # a host-only context chooses no kernels


def test_the_switch_is_refused_after_initialize_with_a_message():
    k = host_context(False)
    k.initialize()
    with pytest.raises(KktError, match=r"cxk_set_streamed_cones.*finalized"):
        k.set_streamed_cones()
    with pytest.raises(KktError, match=r"cxk_set_streamed_cones.*finalized"):
        k.set_streamed_cones(False)
