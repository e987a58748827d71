"""Linear-inequality blocks on the sparse route (kernels_linear_sparse.hip.h), at the edges of the new path, against
the extended-precision reference of cone_reference.py.

The stages and the bounds are those of test_gpu_cone_kernel_matrix.py (run_rows / C_SCHUR, C_PREPARE, C_AFFINE,
C_TAKE, imported): each row runs at the three scaling points through assemble -> constraint_schur -> eigenvalue
query -> PrepareStep -> TakeStep -> affine update on a KktContext whose constructor calls set_sparse_linear(1).
test_linear_sparse_reference.py runs the same rows on the float64 oracle, which shows that correct float64 code
meets the unchanged bounds on them.

The blocks carry a pattern each (make_pattern); test_rows_sit_on_their_edges recomputes every edge with the launch
site's arithmetic, so that a row cannot leave its edge unnoticed.
"""
import ctypes as C

import numpy as np
import pytest

import cone_reference as ref
import conex_api as ca
import oracle_lib as ol
import test_gpu_cone_kernel_matrix as km
import test_gpu_linear_tiled as lt
from conex_amd import KktContext
from conex_amd import synthetic as syn
from conex_amd.kkt import KktError
from test_gpu_parity import blocks, check_newton_step

pytestmark = pytest.mark.gpu

ROW_TILE = 256        # kLinTiledRowTile: rows of the slack one workgroup forms
COL_CHUNK = 4096      # kLinSparseColChunk: entries of a column of G one workgroup holds in LDS
WAVE_COLS = 512       # kLinSparseWaveCols: widest block whose columns one wavefront each assembles
LANES = 64            # entries of a row, and rows of a column, a wavefront takes at a time
LDS_MAX_VARS = 4096   # kLinearLdsMaxVars
MIN_RATIO = 7.8       # kSparseLinearMinRatio
MIN_WORK = 2000 * 64 * 64   # kSparseLinearMinWork: automatic mode moves nothing below this rows m^2

# (id, pattern, K, rows, m)
ROWS = [
    ("min", "dense", 1, 1, 1),                # smallest block
    ("dense-7x5", "dense", 2, 7, 5),          # nnz = rows m on the sparse kernels
    ("holes", "holes", 2, 9, 6),              # an empty row, an empty column
    ("bounds", "bounds", 2, 130, 65),         # [I; -I]: one nonzero per row; m one past the lanes of a wavefront
    ("row-tile", "half", 2, 256, 3),          # exactly one row tile
    ("row-tile-plus-1", "half", 2, 257, 3),   # one row in the second tile
    ("dense-col", "dense-col", 1, 513, 40),   # a column chain over three tiles' rows, nine batches of 64 rows
    ("dense-row", "dense-row", 1, 40, 513),   # a row of nine lane groups; first m on the 256-thread assembly
    ("group-of-3", "half", 3, 300, 65),       # three patterns, three nnz, ragged pointers
    ("wide", "dense-row", 1, 3, 4097),        # first m the LDS route cannot launch; one entry in the second LDS chunk
    ("short-step", "half", 2, 700, 9),        # y eight times the usual: the step is below 1, TakeStep scales d
]
ROW_IDS = [r[0] for r in ROWS]
SHORT_STEP_ROWS = ("short-step",)
POINT_IDS = lt.POINT_IDS


class SparseContext(KktContext):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.set_sparse_linear(1)


class TiledContext(KktContext):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.set_tiled_linear(1)
        self.set_sparse_linear(0)


# ------------------------------------------------------------------------------------ patterns
def scattered(rng, rows, cols, per_row):
    """rows x cols with `per_row` uniform entries per row in distinct columns."""
    A = np.zeros((rows, cols))
    for r in range(rows):
        pick = rng.choice(cols, size=min(per_row, cols), replace=False)
        A[r, pick] = rng.uniform(-1, 1, len(pick))
    return A


def make_pattern(pattern, rows, m, rng):
    if pattern == "dense":
        return rng.uniform(-1, 1, (rows, m))
    if pattern == "half":
        return rng.uniform(-1, 1, (rows, m)) * (rng.random((rows, m)) < 0.5)
    if pattern == "bounds":
        assert rows == 2 * m
        return np.vstack([np.eye(m), -np.eye(m)])
    A = np.zeros((rows, m))
    if pattern == "holes":      # the last column empty, the middle row zeroed
        A[:, :m - 1] = scattered(rng, rows, m - 1, 3)
        A[rows // 2] = 0.0
    elif pattern == "dense-col":
        A[:, 1:] = scattered(rng, rows, m - 1, 2)
        A[:, 0] = rng.uniform(-1, 1, rows)
    elif pattern == "dense-row":
        A[:] = scattered(rng, rows, m, 2)
        A[-1] = rng.uniform(-1, 1, m)
    else:
        raise ValueError(pattern)
    return A


def row_seed(row):
    return 7000 + 31 * row[3] + row[4]


def make_problem(row, point):
    """K equal-shaped blocks, each with its own draw of the row's pattern, on a chain of cliques."""
    _, pattern, K, rows, m = row
    rng = np.random.default_rng(row_seed(row))
    cliques, num_vars = syn.chain_cliques(K, m, 1 if m > 1 else 0)
    cones = []
    for _ in range(K):
        cn = km.make_cone("lin", rows, m, None, point, rng)
        cn["A"] = make_pattern(pattern, rows, m, rng)
        cones.append(cn)
    return cones, cliques, num_vars


def row_problem(row_id, point):
    row = ROWS[ROW_IDS.index(row_id)]
    cones, cliques, num_vars = make_problem(row, point)
    return row, cones, cliques, num_vars, km.make_y(cones, cliques, num_vars, row_seed(row) + 1)


def row_tiles(rows):
    return (rows + ROW_TILE - 1) // ROW_TILE


def col_chunks(m):
    """LaunchLinearSparseSchur, restated: (threads, chunks of a column)."""
    return (64, 1) if m <= WAVE_COLS else (256, (m + COL_CHUNK - 1) // COL_CHUNK)


def lane_groups(n):
    return (n + LANES - 1) // LANES


def test_rows_sit_on_their_edges():
    shape = {r[0]: (r[1], r[2], r[3], r[4]) for r in ROWS}
    assert shape["min"] == ("dense", 1, 1, 1)
    pat, K, rows, m = shape["dense-7x5"]
    assert pat == "dense" and K > 1 and np.count_nonzero(make_problem(ROWS[1], "well")[0][0]["A"]) == rows * m
    pat, K, rows, m = shape["holes"]
    A = make_problem(ROWS[ROW_IDS.index("holes")], "well")[0][0]["A"]
    assert not A[:, m - 1].any() and not A[rows // 2].any() and A[:, :m - 1].any(axis=0).all()
    pat, K, rows, m = shape["bounds"]
    assert pat == "bounds" and rows == 2 * m and m == LANES + 1
    pat, K, rows, m = shape["row-tile"]
    assert K > 1 and rows == ROW_TILE and row_tiles(rows) == 1
    pat, K, rows, m = shape["row-tile-plus-1"]
    assert K > 1 and rows == ROW_TILE + 1 and row_tiles(rows) == 2
    pat, K, rows, m = shape["dense-col"]
    assert pat == "dense-col" and row_tiles(rows) == 3 and row_tiles(rows - 1) == 2
    assert lane_groups(rows) == 9 and lane_groups(rows - 1) == 8  # the column's rows, 64 at a time
    pat, K, rows, m = shape["dense-row"]
    assert pat == "dense-row" and m == WAVE_COLS + 1 and col_chunks(m) == (256, 1) and col_chunks(m - 1) == (64, 1)
    assert lane_groups(m) == 9
    pat, K, rows, m = shape["group-of-3"]
    assert K == 3 and pat == "half" and row_tiles(rows) == 2 and m == LANES + 1
    nnz = [np.count_nonzero(cn["A"]) for cn in make_problem(ROWS[ROW_IDS.index("group-of-3")], "well")[0]]
    assert len(set(nnz)) == 3
    pat, K, rows, m = shape["wide"]
    assert m == LDS_MAX_VARS + 1 and m == COL_CHUNK + 1 and col_chunks(m) == (256, 2) and col_chunks(m - 1) == (256, 1)
    assert set(SHORT_STEP_ROWS) <= set(shape)
    assert max(r[3] for r in ROWS) <= 3073  # (the oracle's own sequential sums pass c = 64 beyond that)


@pytest.mark.parametrize("point", km.POINTS, ids=POINT_IDS)
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_sparse_kernel_matrix(row, point):
    cones, cliques, num_vars = make_problem(row, point)
    counted = []

    class Counting(SparseContext):
        def initialize(self):
            r = super().initialize()
            counted.append((self.count_sparse_linear(), self.count_tiled_linear()))
            return r

    km.run_rows(Counting, cones, cliques, num_vars, row_seed(row) + 1, short_step=row[0] in SHORT_STEP_ROWS, device=0)
    assert counted == [(row[2], 0)]


# ------------------------------------------------------------------------------------ the CSR entry point
def csr_of(A, rng, zeros=3):
    """The nonzeros of A by rows, each row's columns shuffled, with a few explicit zeros at unused positions."""
    rowptr, col, val = [0], [], []
    left = zeros
    for r in range(A.shape[0]):
        nz = list(np.flatnonzero(A[r]))
        vals = [A[r, j] for j in nz]
        free = [j for j in range(A.shape[1]) if A[r, j] == 0.0]
        if left and free:
            nz.append(free[0])
            vals.append(0.0)
            left -= 1
        order = rng.permutation(len(nz))
        col += [int(nz[i]) for i in order]
        val += [float(vals[i]) for i in order]
        rowptr.append(len(col))
    return rowptr, col, val


def build_csr(cones, cliques, num_vars, rng, cls=SparseContext):
    k = cls(num_vars, device=0)
    for i, (cn, cl) in enumerate(zip(cones, cliques)):
        assert k.add_linear_csr(*csr_of(cn["A"], rng), cn["c"], cl) == i
    k.initialize()
    return k


@pytest.mark.parametrize("row_id", ["holes", "group-of-3"])
def test_the_csr_entry_point_gives_the_bits_of_the_dense_one(row_id):
    row, cones, cliques, num_vars, y = row_problem(row_id, 1e6)
    dense = km.build(SparseContext, cones, cliques, num_vars, device=0)
    csr = build_csr(cones, cliques, num_vars, np.random.default_rng(12))
    assert dense.count_sparse_linear() == row[2] and csr.count_sparse_linear() == row[2]
    out = []
    for k in (dense, csr):
        km.set_points(k, cones)
        k.assemble()
        slab, res = k.slab(), k.residuals()
        k.prepare_step(y, km.C_WEIGHT, 1.0)
        k.take_step(0.7, 1.0)
        out.append((slab, res, [k.get_W(i) for i in range(len(cones))]))
    assert np.array_equal(out[0][0], out[1][0])
    assert all(np.array_equal(a, b) for a, b in zip(out[0][1], out[1][1]))
    assert all(np.array_equal(a, b) for a, b in zip(out[0][2], out[1][2]))


def test_a_csr_block_under_mode_0_is_refused_at_initialize():
    rng = np.random.default_rng(4)
    A = make_pattern("half", 20, 10, rng)
    k = KktContext(10, device=0)
    k.set_sparse_linear(0)
    assert k.add_linear_csr(*csr_of(A, rng), np.ones(20)) == 0
    with pytest.raises(KktError, match=r"cxk_add_linear_csr.*sparse route.*cxk_set_sparse_linear"):
        k.initialize()
    k = KktContext(10, device=0)  # the device default is mode 0 too
    assert k.add_linear_csr(*csr_of(A, rng), np.ones(20)) == 0
    with pytest.raises(KktError, match=r"cxk_add_linear_csr"):
        k.initialize()


# ------------------------------------------------------------------------------------ zeros and symmetry
def test_an_empty_variable_gets_exact_zeros_and_g_is_exactly_symmetric():
    row, cones, cliques, num_vars, y = row_problem("holes", 1e6)
    k = km.build(SparseContext, cones, cliques, num_vars, device=0)
    km.set_points(k, cones)
    k.assemble()
    m = row[4]
    for i in range(len(cones)):
        G, AW, AQc, _ = k.constraint_schur(i)
        assert not G[m - 1, :].any() and not G[:, m - 1].any() and AW[m - 1] == 0.0 and AQc[m - 1] == 0.0
        assert np.array_equal(G, G.T) and G[:m - 1, :m - 1].any()


def test_g_of_three_patterns_is_exactly_symmetric():
    row, cones, cliques, num_vars, y = row_problem("group-of-3", 1e6)
    k = km.build(SparseContext, cones, cliques, num_vars, device=0)
    km.set_points(k, cones)
    k.assemble()
    for i in range(len(cones)):
        G = k.constraint_schur(i)[0]
        assert np.array_equal(G, G.T) and G.any()


# ------------------------------------------------------------------------------------ same bits, same results
def test_two_runs_give_the_same_bits():
    row, cones, cliques, num_vars, y = row_problem("dense-col", 1e6)
    k = km.build(SparseContext, cones, cliques, num_vars, device=0)
    assert k.count_sparse_linear() == row[2]
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


@pytest.mark.parametrize("row_id", ["row-tile-plus-1", "group-of-3", "bounds"])
def test_the_sparse_and_the_tiled_route_agree(row_id):
    """Per-row values and the tile partials are the tiled route's bit for bit, and the finish kernels are shared:
    everything behind the slack is equal; the slabs are within 2 C u |.| of each other."""
    row, cones, cliques, num_vars, y = row_problem(row_id, 1e6)
    tiled = km.build(TiledContext, cones, cliques, num_vars, device=0)
    sparse = km.build(SparseContext, cones, cliques, num_vars, device=0)
    assert (tiled.count_tiled_linear(), tiled.count_sparse_linear()) == (row[2], 0)
    assert (sparse.count_tiled_linear(), sparse.count_sparse_linear()) == (0, row[2])
    slabs, outs = [], []
    for k in (tiled, sparse):
        km.set_points(k, cones)
        k.assemble()
        slabs.append(blocks(k, k.slab()))
        query = np.array(k.weighted_slack_eigenvalues(y, km.C_WEIGHT))
        k.prepare_step(y, km.C_WEIGHT, 0.3, affine=1)
        w_affine = [k.get_W(i) for i in range(len(cones))]
        km.set_points(k, cones)
        info = np.array(k.prepare_step(y, km.C_WEIGHT, 1.0))
        per = k.step_info()
        k.take_step(0.7, 1.0)
        outs.append((query, w_affine, info, per, [k.get_W(i) for i in range(len(cones))]))
    mag = lt.magnitude_slab(cones, cliques, num_vars)
    assert np.all(np.abs(slabs[0] - slabs[1]) <= 2 * km.C_SCHUR * km.U * mag)
    a, b = outs
    assert np.array_equal(a[0], b[0])  # lmin, lmax, frob, trace
    assert all(np.array_equal(p, q) for p, q in zip(a[1], b[1]))  # W after the affine PrepareStep
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])  # normsqrd, norminfd, reduced and per constraint
    assert all(np.array_equal(p, q) for p, q in zip(a[4], b[4]))  # W after PrepareStep + take_step(0.7)


def test_prepare_take_step_takes_sparse_blocks():
    row, cones, cliques, num_vars, y = row_problem("group-of-3", "well")
    out = []
    for one_call in (False, True):
        k = km.build(SparseContext, cones, cliques, num_vars, device=0)
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
LS_CASES = [(257, 3, 255), (257, 3, 256), lt.LS_WIDE]  # rows, m, binding row
LS_SEED = 5


def line_search_expected(r, m, bind, b_scaling=0.9, c_scaling=0.8):
    """km.line_search_expected / lt.wide_line_search_expected with half the non-binding entries of A zeroed; the
    three preconditions under which a wrong row is distinguishable from rounding are theirs."""
    rng = np.random.default_rng(LS_SEED + r + bind + m)
    A = rng.uniform(-1, 1, (r, m))
    keep = rng.random((r, m)) < 0.5
    keep[bind] = True
    A *= keep
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


@pytest.mark.parametrize("r,m,bind", LS_CASES)
def test_line_search_takes_the_binding_row(r, m, bind):
    cones, cliques, num_vars, b, dinf, want, (bs, cs) = line_search_expected(r, m, bind)
    assert want > 0
    got = []
    for cls in (SparseContext, TiledContext):
        k = km.build(cls, cones, cliques, num_vars, device=0)
        assert k.count_sparse_linear() == (cls is SparseContext) and k.count_tiled_linear() == (cls is TiledContext)
        km.set_points(k, cones)
        k.set_cost(b)
        k.assemble()
        assert k.factor() == 1
        got.append(k.line_search(dinf, bs, cs))
        assert k.line_search(1e-6, bs, cs) == -1.0  # an interval no step fits
    assert abs(got[0] - float(want)) <= 1e-9 * abs(float(want)), (got, float(want))
    assert got[0] == got[1]


# ------------------------------------------------------------------------------------ the switch
def one_block(k, pattern, m=10):
    rng = np.random.default_rng(3)
    rows = 2 * m
    assert k.add_linear(make_pattern(pattern, rows, m, rng), np.abs(rng.uniform(-1, 1, rows)) + 0.1) == 0
    k.initialize()
    return k


def with_mode(mode, tiled=None, m=10):
    k = KktContext(m, device=0)
    if mode is not None:
        k.set_sparse_linear(mode)
    if tiled is not None:
        k.set_tiled_linear(tiled)
    return k


AUTO_M = 256  # 512 x 256: the smallest [I; -I] the rule was measured on, above the floor on rows m^2


def test_the_device_default_is_mode_0():
    assert one_block(with_mode(None), "bounds").count_sparse_linear() == 0
    assert one_block(with_mode(1), "dense").count_sparse_linear() == 1
    assert one_block(with_mode(0), "bounds").count_sparse_linear() == 0


def test_the_environment_switch_equals_the_call(monkeypatch):
    monkeypatch.setenv("CXK_SPARSE_LINEAR", "1")
    assert one_block(with_mode(None), "dense").count_sparse_linear() == 1
    assert one_block(with_mode(0), "dense").count_sparse_linear() == 0  # an explicit call wins
    monkeypatch.setenv("CXK_SPARSE_LINEAR", "0")
    assert one_block(with_mode(None), "bounds").count_sparse_linear() == 0
    assert one_block(with_mode(1), "bounds").count_sparse_linear() == 1


def test_automatic_mode_moves_a_bounds_block_and_leaves_a_dense_one():
    m = AUTO_M
    assert 2 * m * m * m >= MIN_WORK and MIN_RATIO > 1.0
    k = one_block(with_mode(-1, m=m), "bounds", m)
    assert (k.count_sparse_linear(), k.count_tiled_linear()) == (1, 0)
    k = one_block(with_mode(-1, m=m), "dense", m)
    assert k.count_sparse_linear() == 0
    assert 2 * 10 ** 3 < MIN_WORK  # below the floor nothing moves
    assert one_block(with_mode(-1), "bounds").count_sparse_linear() == 0


def test_the_ratio_of_automatic_mode_can_be_moved(monkeypatch):
    """A dense block has sum nnz_r^2 = rows m^2: it moves at ratio 1 and not one unit above; [I; -I] has
    rows m^2 / sum nnz_r^2 = m^2."""
    m = AUTO_M
    monkeypatch.setenv("CXK_SPARSE_LINEAR_MIN_RATIO", "1")
    assert one_block(with_mode(-1, m=m), "dense", m).count_sparse_linear() == 1
    monkeypatch.setenv("CXK_SPARSE_LINEAR_MIN_RATIO", "2")
    assert one_block(with_mode(-1, m=m), "dense", m).count_sparse_linear() == 0
    monkeypatch.setenv("CXK_SPARSE_LINEAR_MIN_RATIO", str(m * m))
    assert one_block(with_mode(-1, m=m), "bounds", m).count_sparse_linear() == 1
    monkeypatch.setenv("CXK_SPARSE_LINEAR_MIN_RATIO", str(m * m + 1))
    assert one_block(with_mode(-1, m=m), "bounds", m).count_sparse_linear() == 0


@pytest.mark.parametrize("tiled", [0, 1])
def test_an_explicit_tiled_mode_keeps_automatic_off(tiled, monkeypatch):
    m = AUTO_M
    k = one_block(with_mode(-1, tiled, m=m), "bounds", m)
    assert (k.count_sparse_linear(), k.count_tiled_linear()) == (0, tiled)
    monkeypatch.setenv("CXK_TILED_LINEAR", str(tiled))
    k = one_block(with_mode(-1, m=m), "bounds", m)
    assert (k.count_sparse_linear(), k.count_tiled_linear()) == (0, tiled)
    k = one_block(with_mode(1, m=m), "bounds", m)  # mode 1 is not automatic
    assert (k.count_sparse_linear(), k.count_tiled_linear()) == (1, 0)


def test_a_block_over_4097_variables_with_tiled_mode_0():
    m = LDS_MAX_VARS + 1
    A = np.zeros((2, m))
    A[0, 0] = A[1, m - 1] = 0.5
    k = KktContext(m, device=0)
    k.set_tiled_linear(0)
    k.set_sparse_linear(1)
    assert k.add_linear(A, np.ones(2)) == 0
    k.initialize()
    assert (k.count_sparse_linear(), k.count_tiled_linear()) == (1, 0)
    k = KktContext(m, device=0)
    k.set_tiled_linear(0)
    k.set_sparse_linear(0)
    assert k.add_linear(A, np.ones(2)) == 0
    with pytest.raises(KktError, match=r"4096 variables.*cxk_set_tiled_linear"):
        k.initialize()


# ------------------------------------------------------------------------------------ a mixed context
def tall_bounds(rows, m):
    """One +-1 per row, the sign changing with every pass over the variables: bounds on m variables, `rows` tall."""
    A = np.zeros((rows, m))
    r = np.arange(rows)
    A[r, r % m] = np.where((r // m) % 2 == 0, 1.0, -1.0)
    return A


def test_mixed_context():
    """One sparse block (bounds, 130 x 12, added by its nonzeros), one LDS-route block (20 x 12, dense, which automatic
    mode leaves where it is) and one second-order cone over the same variables: the Newton step stage by stage
    against the oracle."""
    m = 12
    rng = np.random.default_rng(92)
    cones = [km.make_cone("lin", 130, m, None, "well", rng), km.make_cone("lin", 20, m, None, "well", rng),
             km.make_cone("soc", 10, m, None, "well", rng)]
    cones[0]["A"] = tall_bounds(130, m)
    cliques = [list(range(m))] * 3
    k = KktContext(m, device=0)
    k.set_sparse_linear(-1)
    assert k.add_linear_csr(*csr_of(cones[0]["A"], rng), cones[0]["c"], cliques[0]) == 0
    assert k.add_linear(cones[1]["A"], cones[1]["c"], cliques[1]) == 1
    assert k.add_soc(cones[2]["A"], cones[2]["c"], cliques[2]) == 2
    k.initialize()
    assert (k.count_sparse_linear(), k.count_tiled_linear()) == (1, 0)
    o = km.build(ol.Program, cones, cliques, m)
    km.set_points(k, cones)
    km.set_points(o, cones)
    check_newton_step(o, k, rng.uniform(-1, 1, m))


# ------------------------------------------------------------------------------------ end to end
LP_ROWS, LP_VARS = lt.LP_ROWS, lt.LP_VARS


def lp_data():
    """lt.lp_data with half of A's entries zeroed, and finite bounds on every variable."""
    rng = np.random.default_rng(2028)
    A = rng.uniform(-1, 1, (LP_ROWS, LP_VARS)) * (rng.random((LP_ROWS, LP_VARS)) < 0.5)
    c = np.abs(rng.uniform(-1, 1, LP_ROWS))
    x0 = np.abs(rng.uniform(-1, 1, LP_ROWS))
    x0 *= 0.01 / np.linalg.norm(x0)
    lb, ub = -rng.uniform(0.5, 1.5, LP_VARS), rng.uniform(0.5, 1.5, LP_VARS)
    return A, c, A.T @ x0, lb, ub


def bounds_rows(lb, ub):
    """What CONEX_AddLinearInequalities makes of lb <= I y <= ub: per variable the scaled upper, then lower row."""
    n = len(lb)
    A, c = np.zeros((2 * n, n)), np.zeros(2 * n)
    for i in range(n):
        su, sl = 1.0 / np.sqrt(1.0 + ub[i] * ub[i]), 1.0 / np.sqrt(1.0 + lb[i] * lb[i])
        A[2 * i, i], c[2 * i] = su, su * ub[i]
        A[2 * i + 1, i], c[2 * i + 1] = -sl, -sl * lb[i]
    return A, c


def lp_oracle(cfg):
    A, c, b, lb, ub = lp_data()
    o = ol.Program(LP_VARS)
    o.add_linear(*bounds_rows(lb, ub))
    o.add_linear(A, c)
    ocfg = ol.default_config()
    for f, _ in ocfg._fields_:
        setattr(ocfg, f, getattr(cfg, f))
    return o.solve(b, ocfg)


def lp_device(cfg, mode):
    A, c, b, lb, ub = lp_data()
    L = ca.api()
    p = L.CONEX_CreateConeProgram()
    assert L.CONEX_HIP_SetSparseLinear(p, mode) == 0
    eye = np.eye(LP_VARS)
    # (the call reports -1 whatever it did, as the reference's does)
    assert L.CONEX_AddLinearInequalities(p, ca.dp(ca.colmajor(eye)), LP_VARS, LP_VARS, ca.dp(lb), LP_VARS, ca.dp(ub), LP_VARS) == -1
    assert L.CONEX_AddDenseLinearConstraint(p, ca.dp(ca.colmajor(A)), LP_ROWS, LP_VARS, ca.dp(c), LP_ROWS) == 1  # (its constraint number)
    y = np.zeros(LP_VARS)
    ok = L.CONEX_Maximize(p, ca.dp(np.ascontiguousarray(b)), LP_VARS, C.byref(cfg), ca.dp(y), LP_VARS)
    L.CONEX_DeleteConeProgram(p)
    return ok, y


@pytest.mark.parametrize("line_search", [0, 1], ids=["mu-rule", "line-search"])
def test_an_lp_through_conex_h_on_both_modes(line_search):
    cfg = lt.lp_config(line_search)
    oko, yo = lp_oracle(cfg)
    ok1, y1 = lp_device(cfg, 1)
    ok0, y0 = lp_device(cfg, 0)
    assert oko == 1 and ok1 == 1 and ok0 == 1
    scale = np.linalg.norm(yo)
    assert np.linalg.norm(y1 - y0) <= 1e-6 * scale
    assert np.linalg.norm(y1 - yo) <= 1e-6 * scale and np.linalg.norm(y0 - yo) <= 1e-6 * scale
