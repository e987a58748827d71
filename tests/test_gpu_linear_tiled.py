"""Linear-inequality blocks on the tiled route (kernels_linear_tiled.hip.h), at the edges of the new path,
against the extended-precision reference of cone_reference.py.

The problems, the stages and the bounds are those of test_gpu_cone_kernel_matrix.py (make_problem / run_rows /
C_SCHUR, C_PREPARE, C_AFFINE, C_TAKE, imported): each row runs at the three scaling points through assemble ->
constraint_schur -> eigenvalue query -> PrepareStep -> TakeStep -> affine update on a KktContext whose constructor
calls set_tiled_linear(1).  test_linear_tiled_reference.py runs the same rows on the float64 oracle, which shows
that correct float64 code meets the bounds at these lengths too (its worst quantity reaches about half of its
bound; a block of 5000 rows did not pass, which is why no row is longer than 3073).

Each row is the smallest shape at which its mechanism first engages; test_rows_sit_on_their_edges recomputes
every edge with the launch site's arithmetic, so that a row cannot leave its edge unnoticed.
"""
import ctypes as C

import numpy as np
import pytest

import cone_reference as ref
import conex_api as ca
import oracle_lib as ol
import test_gpu_cone_kernel_matrix as km
from conex_amd import KktContext
from conex_amd.kkt import KktError
from test_gpu_parity import blocks, check_newton_step

pytestmark = pytest.mark.gpu

ROW_TILE = 256          # kLinTiledRowTile
Y_CHUNK = 2048          # kLinTiledYChunk
MIN_SPLIT_K = 1024      # kSocStreamMinSplitK (the Gram product's split rule is the streamed cones')
GEMM_TILE = 64          # kGemmBM = kGemmBN
MFMA_TILE = 16          # v_mfma_f64_16x16x4_f64
LDS_DEFAULT = 65536     # dynamic LDS a kernel may ask for without the attribute
LDS_MAX_VARS = 4096     # kLinearLdsMaxVars

# (id, kind, K, rows, m, extra) as km.ROWS
ROWS = [
    ("min", "lin", 1, 1, 1, None),                # smallest block; the GEMM with M = N = K = 1; lanes without rows
    ("row-tile", "lin", 2, 256, 3, None),         # exactly one row tile
    ("row-tile-plus-1", "lin", 2, 257, 3, None),  # one row in the second tile: a partly empty tile in min / max
    ("below-split-k", "lin", 1, 2047, 17, None),  # last unsplit length; m one past an MFMA tile
    ("split-k", "lin", 1, 2048, 17, None),        # first length whose Gram product is split in two
    ("split-ragged", "lin", 1, 3073, 5, None),    # three pieces of unequal length, odd rows (the GEMM's general kernel)
    ("group-of-3", "lin", 3, 300, 65, None),      # batch of three; m one past a 64-wide GEMM tile
    ("two-gemm-tiles", "lin", 2, 260, 129, None), # m one past two tiles; one tile of rows plus four
    ("y-chunk", "lin", 1, 3, 2049, None),         # one entry in the second y chunk; fewer rows than a wavefront
    ("wide", "lin", 1, 2, 4097, None),            # third y chunk; first m the LDS route's line search cannot launch
    ("short-step", "lin", 2, 700, 9, None),       # y eight times the usual: the step is below 1, TakeStep scales d
]
ROW_IDS = [r[0] for r in ROWS]
SHORT_STEP_ROWS = ("short-step",)
POINT_IDS = [p if isinstance(p, str) else f"cond{p:.0e}" for p in km.POINTS]
WIDEST = (2, 8193)  # rows, m: first m at which the LDS route's PrepareStep cannot launch either


class TiledContext(KktContext):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.set_tiled_linear(1)


class LdsContext(KktContext):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.set_tiled_linear(0)


def gram_splits(rows, m, count):
    """SocStreamSplits, restated."""
    tiles = ((m + GEMM_TILE - 1) // GEMM_TILE) ** 2 * count
    return max(1, min(rows // MIN_SPLIT_K, (512 + tiles - 1) // tiles))


def row_tiles(rows):
    return (rows + ROW_TILE - 1) // ROW_TILE


def y_chunks(m):
    return (m + Y_CHUNK - 1) // Y_CHUNK


def row_seed(row):
    return 6000 + km.row_seed(row)


def test_rows_sit_on_their_edges():
    shape = {r[0]: (r[2], r[3], r[4]) for r in ROWS}
    assert all(r[1] == "lin" for r in ROWS)
    assert shape["min"] == (1, 1, 1)
    K, rows, m = shape["row-tile"]
    assert K > 1 and rows == ROW_TILE and row_tiles(rows) == 1
    K, rows, m = shape["row-tile-plus-1"]
    assert K > 1 and rows == ROW_TILE + 1 and row_tiles(rows) == 2 and row_tiles(rows - 1) == 1
    K, rows, m = shape["below-split-k"]
    assert m == MFMA_TILE + 1 and gram_splits(rows, m, K) == 1 and gram_splits(rows + 1, m, K) == 2
    K, rows, m = shape["split-k"]
    assert m == MFMA_TILE + 1 and gram_splits(rows, m, K) == 2 and gram_splits(rows - 1, m, K) == 1
    K, rows, m = shape["split-ragged"]
    steps = (rows + 15) // 16  # LaunchGemmSplitK deals whole steps of kGemmBK = 16
    per = (steps + 2) // 3
    assert gram_splits(rows, m, K) == 3 and rows % 2 == 1 and 0 < steps - 2 * per < per
    K, rows, m = shape["group-of-3"]
    assert K == 3 and m == GEMM_TILE + 1 and row_tiles(rows) == 2
    K, rows, m = shape["two-gemm-tiles"]
    assert m == 2 * GEMM_TILE + 1 and rows == ROW_TILE + 4
    K, rows, m = shape["y-chunk"]
    assert m == Y_CHUNK + 1 and y_chunks(m) == 2 and rows < 64
    K, rows, m = shape["wide"]
    assert y_chunks(m) == 3 and m == LDS_MAX_VARS + 1
    assert 8 * 2 * m > LDS_DEFAULT >= 8 * 2 * (m - 1)    # linear_line_search's dynamic LDS
    assert 8 * WIDEST[1] > LDS_DEFAULT >= 8 * (WIDEST[1] - 1)  # linear_prepare's
    unsplit = [r[0] for r in ROWS if gram_splits(r[3], r[4], r[2]) == 1]
    assert set(unsplit) == set(ROW_IDS) - {"split-k", "split-ragged"}
    assert set(SHORT_STEP_ROWS) <= set(shape)
    assert max(r[3] for r in ROWS) == 3073  # (the oracle's own sequential sums pass c = 64 beyond that)


@pytest.mark.parametrize("point", km.POINTS, ids=POINT_IDS)
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_tiled_kernel_matrix(row, point):
    cones, cliques, num_vars = km.make_problem(row, point, row_seed(row))
    counted = []

    class Counting(TiledContext):
        def initialize(self):
            r = super().initialize()
            counted.append(self.count_tiled_linear())
            return r

    km.run_rows(Counting, cones, cliques, num_vars, row_seed(row) + 1, short_step=row[0] in SHORT_STEP_ROWS, device=0)
    assert counted == [row[2]]


# ------------------------------------------------------------------------------------ the widest block
def widest_case(point):
    rows, m = WIDEST
    rng = np.random.default_rng(77)
    cn = km.make_cone("lin", rows, m, None, point, rng)
    cliques = [list(range(m))]
    return cn, cliques, m, km.make_y([cn], cliques, m, 5)


def check_widest(k, cn, y, report=None):
    """The stages that need no 8193 x 8193 download, against the reference at C_PREPARE."""
    q = ref.lin_query(cn["A"], cn["c"], cn["W"], y, km.C_WEIGHT)
    ek = k.weighted_slack_eigenvalues(y, km.C_WEIGHT)
    for j, name in enumerate(("lmin", "lmax", "frob", "trace")):
        km.within(ek[j], *q[name], km.C_PREPARE, f"query {name}", report)
    p = ref.lin_prepare(cn["A"], cn["c"], cn["W"], y, km.C_WEIGHT, 1.0)
    ik = k.prepare_step(y, km.C_WEIGHT, 1.0)
    km.within(ik[0], *p["normsqrd"], km.C_PREPARE, "normsqrd", report)
    km.within(ik[1], *p["norminfd"], km.C_PREPARE, "norminfd", report)
    return report


@pytest.mark.parametrize("point", km.POINTS, ids=POINT_IDS)
def test_the_widest_block_takes_the_tiled_route_by_itself(point):
    """2 rows over 8193 variables in automatic mode: the LDS route's PrepareStep cannot be launched there."""
    cn, cliques, m, y = widest_case(point)
    k = km.build(KktContext, [cn], cliques, m, device=0)
    assert k.count_tiled_linear() == 1
    km.set_points(k, [cn])
    check_widest(k, cn, y)


# ------------------------------------------------------------------------------------ the switch
def small_block(k, rows=20, m=10):
    rng = np.random.default_rng(3)
    assert k.add_linear(rng.uniform(-1, 1, (rows, m)), np.abs(rng.uniform(-1, 1, rows)) + 0.1) == 0
    k.initialize()
    return k


def test_automatic_mode_leaves_a_small_block_on_the_lds_route_and_mode_1_moves_it():
    assert small_block(KktContext(10, device=0)).count_tiled_linear() == 0
    assert small_block(TiledContext(10, device=0)).count_tiled_linear() == 1
    k = KktContext(10, device=0)
    k.set_tiled_linear(-1)
    assert small_block(k).count_tiled_linear() == 0


def test_the_environment_switch_equals_the_call(monkeypatch):
    monkeypatch.setenv("CXK_TILED_LINEAR", "1")
    assert small_block(KktContext(10, device=0)).count_tiled_linear() == 1
    assert small_block(LdsContext(10, device=0)).count_tiled_linear() == 0  # an explicit call wins
    monkeypatch.setenv("CXK_TILED_LINEAR", "0")
    assert small_block(KktContext(10, device=0)).count_tiled_linear() == 0
    assert small_block(TiledContext(10, device=0)).count_tiled_linear() == 1


def test_the_work_threshold_of_automatic_mode_can_be_moved(monkeypatch):
    monkeypatch.setenv("CXK_TILED_LINEAR_MIN_WORK", str(20 * 10 * 10))
    assert small_block(KktContext(10, device=0)).count_tiled_linear() == 1
    monkeypatch.setenv("CXK_TILED_LINEAR_MIN_WORK", str(20 * 10 * 10 + 1))
    assert small_block(KktContext(10, device=0)).count_tiled_linear() == 0


def test_mode_0_refuses_a_block_the_lds_route_cannot_launch():
    m = LDS_MAX_VARS + 1
    k = LdsContext(m, device=0)
    assert k.add_linear(np.full((2, m), 0.01), np.ones(2)) == 0
    with pytest.raises(KktError, match=r"4096 variables.*cxk_set_tiled_linear"):
        k.initialize()
    k = LdsContext(m - 1, device=0)  # the last width it can
    assert k.add_linear(np.full((2, m - 1), 0.01), np.ones(2)) == 0
    k.initialize()
    assert k.count_tiled_linear() == 0


# ------------------------------------------------------------------------------------ same bits, same results
def row_problem(row_id, point):
    row = ROWS[ROW_IDS.index(row_id)]
    cones, cliques, num_vars = km.make_problem(row, point, row_seed(row))
    return row, cones, cliques, num_vars, km.make_y(cones, cliques, num_vars, row_seed(row) + 1)


def test_two_runs_give_the_same_bits():
    row, cones, cliques, num_vars, y = row_problem("split-k", 1e6)
    k = km.build(TiledContext, cones, cliques, num_vars, device=0)
    assert k.count_tiled_linear() == row[2]
    km.set_points(k, cones)
    runs = []
    for _ in range(2):
        k.assemble()
        runs.append((k.slab(), k.residuals()))
    assert np.array_equal(runs[0][0], runs[1][0])
    assert all(np.array_equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    infos = []
    for _ in range(2):
        km.set_points(k, cones)
        ik = k.prepare_step(y, km.C_WEIGHT, 1.0)
        infos.append((ik, k.step_info(), k.weighted_slack_eigenvalues(y, km.C_WEIGHT)))
    assert all(np.array_equal(a, b) for a, b in zip(infos[0], infos[1]))


def magnitude_slab(cones, cliques, num_vars):
    """The slab of sum |w a_ki| |w a_kj|: the magnitude each assembled entry's bound is relative to."""
    mags = [dict(cn, A=np.abs(cn["A"])) for cn in cones]
    o = km.build(ol.Program, mags, cliques, num_vars)
    km.set_points(o, mags)
    o.assemble()
    return blocks(o, o.slab())


@pytest.mark.parametrize("row_id", ["row-tile-plus-1", "split-k", "group-of-3"])
def test_the_two_routes_agree(row_id):
    """Each route is within C u |.| of the reference, so they are within 2 C u |.| of each other."""
    row, cones, cliques, num_vars, y = row_problem(row_id, 1e6)
    lds = km.build(LdsContext, cones, cliques, num_vars, device=0)
    tiled = km.build(TiledContext, cones, cliques, num_vars, device=0)
    assert lds.count_tiled_linear() == 0 and tiled.count_tiled_linear() == row[2]
    slabs = []
    for k in (lds, tiled):
        km.set_points(k, cones)
        k.assemble()
        slabs.append(blocks(k, k.slab()))  # (the entries that are read: lower triangles and off-diagonal blocks)
    mag = magnitude_slab(cones, cliques, num_vars)
    assert np.all(np.abs(slabs[0] - slabs[1]) <= 2 * km.C_SCHUR * km.U * mag)
    for k in (lds, tiled):
        k.prepare_step(y, km.C_WEIGHT, 1.0)
        k.take_step(0.7, 1.0)
    for i, (cn, cl) in enumerate(zip(cones, cliques)):
        _, Wm = ref.lin_take(cn["A"], cn["c"], cn["W"], y[cl], km.C_WEIGHT, 1.0, 0.7)
        assert np.all(np.abs(lds.get_W(i) - tiled.get_W(i)) <= 2 * km.C_TAKE * km.U * np.asarray(Wm, dtype=np.float64))


def test_prepare_take_step_takes_tiled_blocks():
    """The step length is read on the device by linear_take_step behind the tiled PrepareStep too: the one-call form
    takes the step and leaves the W of the two calls, bit for bit."""
    row, cones, cliques, num_vars, y = row_problem("group-of-3", "well")
    out = []
    for one_call in (False, True):
        k = km.build(TiledContext, cones, cliques, num_vars, device=0)
        km.set_points(k, cones)
        if one_call:
            n2, ninf, took = k.prepare_take_step(y, km.C_WEIGHT, 1.0)
            assert took
        else:
            n2, ninf = k.prepare_step(y, km.C_WEIGHT, 1.0)
            k.take_step(min(1.0, 2.0 / ninf ** 2), 1.0)
        out.append((np.array([n2, ninf]), [k.get_W(i) for i in range(len(cones))]))
    assert np.array_equal(out[0][0], out[1][0])
    assert all(np.array_equal(a, b) for a, b in zip(out[0][1], out[1][1]))


# ------------------------------------------------------------------------------------ line search
def run_line_search(expected):
    cones, cliques, num_vars, b, dinf, want, (bs, cs) = expected
    assert want > 0
    k = km.build(TiledContext, cones, cliques, num_vars, device=0)
    assert k.count_tiled_linear() == 1
    km.set_points(k, cones)
    k.set_cost(b)
    k.assemble()
    assert k.factor() == 1
    got = k.line_search(dinf, bs, cs)
    assert abs(got - float(want)) <= 1e-9 * abs(float(want)), (got, float(want))
    assert k.line_search(1e-6, bs, cs) == -1.0  # an interval no step fits


@pytest.mark.parametrize("r,bind", [(257, 255), (257, 256), (1000, 999)])
def test_line_search_takes_the_binding_row(r, bind):
    run_line_search(km.line_search_expected(r, bind))


LS_WIDE = (300, 70, 299)  # rows, m, binding row (in the second row tile)


def wide_line_search_expected(b_scaling=0.9, c_scaling=0.8):
    """km.line_search_problem / line_search_expected with m variables instead of three: the binding row scaled by 6,
    the cost block (r + 40)(R R'/m + I); the precondition under which a wrong row is distinguishable from rounding
    is asserted before anything is asked of the device."""
    r, m, bind = LS_WIDE
    rng = np.random.default_rng(5 + r + bind + m)
    A = rng.uniform(-1, 1, (r, m))
    c = np.abs(rng.uniform(-1, 1, r)) + 0.1
    A[bind] *= 6.0
    c[bind] = 6.0
    R = rng.uniform(-1, 1, (m, m))
    G = (r + 40.0) * (R @ R.T / m + np.eye(m))
    cones = [dict(kind="lin", m=m, A=A, c=c, W=rng.uniform(0.5, 1.0, r)), dict(kind="static", m=m, G=G)]
    cliques, b = [list(range(m))] * 2, rng.uniform(-1, 1, m)
    Y, d0 = km.line_search_reference(cones, cliques, m, b, b_scaling, c_scaling)
    dinf = float(1.5 * np.max(np.abs(d0)))
    lbs, ubs, delta = ref.lin_line_search(A, c, cones[0]["W"], Y[:, 0], Y[:, 1], c_scaling, dinf)
    order = np.argsort(ubs)
    assert order[0] == bind, (order[:3], bind)
    assert abs(delta[bind]) >= 0.1 * np.max(np.abs(delta))
    assert ubs[order[1]] - ubs[bind] >= 1e-3 * abs(ubs[bind])
    return cones, cliques, m, b, dinf, ref.line_search_result([lbs], [ubs]), (b_scaling, c_scaling)


def test_line_search_over_seventy_variables():
    run_line_search(wide_line_search_expected())


# ------------------------------------------------------------------------------------ a mixed context
def test_mixed_context(monkeypatch):
    """One tiled block (600 x 12), one LDS-route block (20 x 12) and one second-order cone over the same variables:
    the Newton step stage by stage against the oracle."""
    m = 12
    rng = np.random.default_rng(91)
    cones = [km.make_cone("lin", 600, m, None, "well", rng), km.make_cone("lin", 20, m, None, "well", rng),
             km.make_cone("soc", 10, m, None, "well", rng)]
    cliques = [list(range(m))] * 3
    monkeypatch.setenv("CXK_TILED_LINEAR_MIN_WORK", str(600 * m * m))
    k = km.build(KktContext, cones, cliques, m, device=0)
    assert k.count_tiled_linear() == 1
    o = km.build(ol.Program, cones, cliques, m)
    km.set_points(k, cones)
    km.set_points(o, cones)
    check_newton_step(o, k, rng.uniform(-1, 1, m))


# ------------------------------------------------------------------------------------ end to end
LP_ROWS, LP_VARS = 600, 40


def lp_data():
    rng = np.random.default_rng(2027)
    A = rng.uniform(-1, 1, (LP_ROWS, LP_VARS))
    c = np.abs(rng.uniform(-1, 1, LP_ROWS))
    x0 = np.abs(rng.uniform(-1, 1, LP_ROWS))
    x0 *= 0.01 / np.linalg.norm(x0)
    return A, c, A.T @ x0


def lp_config(line_search):
    cfg = ca.default_config()
    cfg.inv_sqrt_mu_max = 5e5
    cfg.divergence_upper_bound = 1000
    cfg.dinf_upper_bound = 1.35
    cfg.final_centering_tolerance = 1
    cfg.enable_line_search = int(line_search)
    return cfg


def lp_oracle(cfg):
    A, c, b = lp_data()
    o = ol.Program(LP_VARS)
    o.add_linear(A, c)
    ocfg = ol.default_config()
    for f, _ in ocfg._fields_:
        setattr(ocfg, f, getattr(cfg, f))
    return o.solve(b, ocfg)


def lp_device(cfg, mode):
    A, c, b = lp_data()
    L = ca.api()
    p = L.CONEX_CreateConeProgram()
    assert L.CONEX_HIP_SetTiledLinear(p, mode) == 0
    assert L.CONEX_AddDenseLinearConstraint(p, ca.dp(ca.colmajor(A)), LP_ROWS, LP_VARS, ca.dp(c), LP_ROWS) == 0
    y = np.zeros(LP_VARS)
    ok = L.CONEX_Maximize(p, ca.dp(np.ascontiguousarray(b)), LP_VARS, C.byref(cfg), ca.dp(y), LP_VARS)
    L.CONEX_DeleteConeProgram(p)
    return ok, y


@pytest.mark.parametrize("line_search", [0, 1], ids=["mu-rule", "line-search"])
def test_an_lp_through_conex_h_on_both_routes(line_search):
    cfg = lp_config(line_search)
    oko, yo = lp_oracle(cfg)
    ok1, y1 = lp_device(cfg, 1)
    ok0, y0 = lp_device(cfg, 0)
    assert oko == 1 and ok1 == 1 and ok0 == 1
    scale = np.linalg.norm(yo)
    assert np.linalg.norm(y1 - y0) <= 1e-6 * scale
    assert np.linalg.norm(y1 - yo) <= 1e-6 * scale and np.linalg.norm(y0 - yo) <= 1e-6 * scale
