"""Second-order cones on the sparse route (kernels_soc_sparse.hip.h), at the edges of the new path, against the
extended-precision reference of cone_reference.py.

The stages and the bounds are those of test_gpu_cone_kernel_matrix.py (run_rows / C_SCHUR, C_PREPARE, C_TAKE,
imported): each row runs at the three scaling points through assemble -> constraint_schur -> eigenvalue query ->
PrepareStep -> TakeStep on a KktContext whose constructor calls set_sparse_soc(1).  The step stages are compared with
the second-order cone's reference as everywhere; the Schur stage with cone_reference.quad_schur(A, c, W, None), the
expressions the route evaluates (G = 4 u u' + 2 det(w) A' J A written in w itself: no square root, g = 1), through
the wrapper run_rows below.  test_soc_sparse_reference.py runs the same rows without a GPU.

The cones carry a pattern each (make_pattern); test_rows_sit_on_their_edges recomputes every edge from the launch
site's constants, so that a row cannot leave its edge unnoticed.
"""
import ctypes as C
import re

import numpy as np
import pytest

import cone_reference as ref
import test_gpu_cone_kernel_matrix as km
import test_gpu_linear_sparse as ls
import test_gpu_soc_streamed as ss
from conex_amd import KktContext
from conex_amd import synthetic as syn
from conex_amd.kkt import KktError
from test_sharding import ThreadRanks, _newton_iteration

pytestmark = pytest.mark.gpu

ROW_TILE = 256        # kSocStreamRowTile: rows of the slack one workgroup forms
LANES = 64            # entries of a column a wavefront of soc_sparse_dots / soc_sparse_gram takes at a time
DOT_COLS = 4          # columns one workgroup of soc_sparse_dots takes (kSocSparseBlock / 64)
WAVE_COLS = 512       # kSocSparseWaveCols: widest cone whose columns of H one wavefront each assembles
COL_CHUNK = 4096      # kSocSparseColChunk: entries of a column of H one workgroup holds in LDS
COMBINE_TILE = 1024   # kSocSparseCombineTile: entries of G one workgroup of soc_sparse_combine writes
MIN_RATIO = 4.04      # kSparseSocMinRatio: automatic mode moves a cone from len m / nnz >= this on
MIN_WORK = 2 * 401 * 61 * 61   # kSparseSocMinWork: and nothing below this len m^2

# (id, pattern, K, n, m): the cone has dimension len = n + 1
ROWS = [
    ("least-squares", "lsq", 1, 60, 12),       # |A x - b| <= t: row 0 holds the t column only, the others 2 - 3 entries
    ("empty-column", "empty-col", 2, 30, 7),   # a variable without a nonzero: its row and column of G are exactly 0
    ("empty-row", "empty-row", 2, 30, 7),      # a row without a nonzero
    ("dense-40x9", "dense", 1, 40, 9),         # nnz = len m on the sparse kernels
    ("lds-fit", "half", 2, 10, 10),            # fits LDS: on the sparse route because of mode 1 only
    ("group-of-3", "half", 3, 300, 65),        # three patterns, three nnz, ragged pointers
    ("row-tile", "three", 1, 1280, 15),        # len = 5 x 256 + 1: one row in the last tile of the slack
    ("column-65", "dense-col", 1, 64, 8),      # a column of 65 entries: the lanes' chains wrap once
    ("column-257", "dense-col", 1, 256, 8),    # a column of 257 entries: five batches of 64 rows in soc_sparse_gram
    ("combine-1024", "half", 1, 20, 32),       # m m = 1024: exactly one tile of soc_sparse_combine
    ("combine-1089", "half", 1, 20, 33),       # one tile and 65 entries of a second
    ("wave-512", "dense-row", 1, 40, 512),     # the widest cone on the wavefront-per-column assembly of H
    ("block-513", "dense-row", 1, 40, 513),    # the first on the 256-thread assembly
    ("short-step", "half", 1, 300, 9),         # y eight times the usual: the step is below 1, TakeStep scales d
]
ROW_IDS = [r[0] for r in ROWS]
SHORT_STEP_ROWS = ("short-step",)
POINT_IDS = ls.POINT_IDS
WIDE = ("wide", "dense-row", 1, 3, COL_CHUNK + 1)  # one entry in the second LDS chunk (checked in float64, below)


class SparseSocContext(KktContext):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.set_sparse_soc(1)


class StreamedContext(KktContext):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.set_streamed_cones()
        self.set_sparse_soc(0)


# ------------------------------------------------------------------------------------ patterns
def make_pattern(pattern, n, m, rng):
    """The (n + 1) x m matrix of a cone."""
    rows = n + 1
    if pattern == "dense":
        return rng.uniform(-1, 1, (rows, m))
    if pattern == "half":
        return rng.uniform(-1, 1, (rows, m)) * (rng.random((rows, m)) < 0.5)
    if pattern == "three":
        return ls.scattered(rng, rows, m, 3)
    A = np.zeros((rows, m))
    if pattern == "lsq":          # y = (x, t): row 0 is -t, row r > 0 is -(A x)_r with 2 or 3 entries
        A[0, m - 1] = -1.0
        for r in range(1, rows):
            pick = rng.choice(m - 1, size=2 + r % 2, replace=False)
            A[r, pick] = rng.uniform(-1, 1, len(pick))
    elif pattern == "empty-col":  # the last column empty
        A[:, :m - 1] = ls.scattered(rng, rows, m - 1, 3)
    elif pattern == "empty-row":  # the middle row zeroed
        A[:] = ls.scattered(rng, rows, m, 3)
        A[rows // 2] = 0.0
    elif pattern == "dense-col":
        A[:, 1:] = ls.scattered(rng, rows, m - 1, 2)
        A[:, 0] = rng.uniform(-1, 1, rows)
    elif pattern == "dense-row":
        A[:] = ls.scattered(rng, rows, m, 2)
        A[-1] = rng.uniform(-1, 1, m)
    else:
        raise ValueError(pattern)
    return A


def row_seed(row):
    return 9000 + 31 * row[3] + row[4]


def make_problem(row, point):
    """K equal-shaped cones, each with its own draw of the row's pattern, on a chain of cliques."""
    _, pattern, K, n, m = row
    rng = np.random.default_rng(row_seed(row))
    cliques, num_vars = syn.chain_cliques(K, m, 1 if m > 1 else 0)
    cones = []
    for _ in range(K):
        cn = km.make_cone("soc", n, m, None, point, rng)
        cn["A"] = make_pattern(pattern, n, m, rng)
        cones.append(cn)
    return cones, cliques, num_vars


def row_problem(row_id, point):
    row = ROWS[ROW_IDS.index(row_id)]
    cones, cliques, num_vars = make_problem(row, point)
    return row, cones, cliques, num_vars, km.make_y(cones, cliques, num_vars, row_seed(row) + 1)


def sparse_schur_reference(cn, others=km.ref_schur):
    """The Schur stage's reference on the sparse route: the expressions it evaluates, in longdouble, g = 1."""
    if cn["kind"] == "soc":
        return ref.quad_schur(cn["A"], cn["c"], cn["W"], None)
    return others(cn)


def run_rows(cls, cones, cliques, num_vars, seed, report=None, short_step=False, **kw):
    """km.run_rows with the Schur stage of the second-order cones compared against sparse_schur_reference."""
    saved = km.ref_schur
    km.ref_schur = lambda cn: sparse_schur_reference(cn, saved)
    try:
        return km.run_rows(cls, cones, cliques, num_vars, seed, report, short_step=short_step, **kw)
    finally:
        km.ref_schur = saved


def row_tiles(length):
    return (length + ROW_TILE - 1) // ROW_TILE


def gram_shape(m):
    """SocSparseConstants, restated: (threads, chunks of a column of H)."""
    return (64, 1) if m <= WAVE_COLS else (256, (m + COL_CHUNK - 1) // COL_CHUNK)


def combine_tiles(m):
    return (m * m + COMBINE_TILE - 1) // COMBINE_TILE


def lane_groups(n):
    return (n + LANES - 1) // LANES


def test_rows_sit_on_their_edges():
    shape = {r[0]: (r[1], r[2], r[3], r[4]) for r in ROWS}
    first = {rid: make_problem(ROWS[ROW_IDS.index(rid)], "well")[0] for rid in
             ("least-squares", "empty-column", "empty-row", "dense-40x9", "group-of-3", "column-65", "column-257")}
    pat, K, n, m = shape["least-squares"]
    A = first["least-squares"][0]["A"]
    per_row = np.count_nonzero(A, axis=1)
    assert np.flatnonzero(A[0]).tolist() == [m - 1] and not A[1:, m - 1].any() and set(per_row[1:]) == {2, 3}
    pat, K, n, m = shape["empty-column"]
    A = first["empty-column"][0]["A"]
    assert not A[:, m - 1].any() and A[:, :m - 1].any(axis=0).all() and A.any(axis=1).all()
    pat, K, n, m = shape["empty-row"]
    A = first["empty-row"][0]["A"]
    assert not A[(n + 1) // 2].any() and A.any(axis=0).all()
    pat, K, n, m = shape["dense-40x9"]
    assert (n, m) == (40, 9) and np.count_nonzero(first["dense-40x9"][0]["A"]) == (n + 1) * m
    pat, K, n, m = shape["lds-fit"]
    assert (n, m) == (10, 10) and ss.staged(n, m)
    assert all(not ss.staged(r[3], r[4]) for r in ROWS if r[0] in ("row-tile", "wave-512", "block-513"))
    pat, K, n, m = shape["group-of-3"]
    assert K == 3 and len({np.count_nonzero(cn["A"]) for cn in first["group-of-3"]}) == 3
    assert (K * m) % DOT_COLS != 0  # the last workgroup of soc_sparse_dots has idle wavefronts
    pat, K, n, m = shape["row-tile"]
    assert (n + 1) % ROW_TILE == 1 and row_tiles(n + 1) == 6 and row_tiles(n) == 5
    for rid, entries in (("column-65", LANES + 1), ("column-257", 4 * LANES + 1)):
        pat, K, n, m = shape[rid]
        A = first[rid][0]["A"]
        assert np.count_nonzero(A[:, 0]) == n + 1 == entries and lane_groups(n + 1) == lane_groups(n) + 1
    pat, K, n, m = shape["combine-1024"]
    assert m * m == COMBINE_TILE and combine_tiles(m) == 1
    pat, K, n, m = shape["combine-1089"]
    assert combine_tiles(m) == 2 and combine_tiles(m - 1) == 1
    pat, K, n, m = shape["wave-512"]
    assert pat == "dense-row" and m == WAVE_COLS and gram_shape(m) == (64, 1)
    pat, K, n, m = shape["block-513"]
    assert pat == "dense-row" and m == WAVE_COLS + 1 and gram_shape(m) == (256, 1) and lane_groups(m) == 9
    _, pat, K, n, m = WIDE
    assert m == COL_CHUNK + 1 and gram_shape(m) == (256, 2) and gram_shape(m - 1) == (256, 1)
    assert set(SHORT_STEP_ROWS) <= set(shape)


@pytest.mark.parametrize("point", km.POINTS, ids=POINT_IDS)
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_sparse_kernel_matrix(row, point):
    cones, cliques, num_vars = make_problem(row, point)
    counted = []

    class Counting(SparseSocContext):
        def initialize(self):
            r = super().initialize()
            counted.append((self.count_sparse_soc(), self.count_streamed_cones()))
            return r

    run_rows(Counting, cones, cliques, num_vars, row_seed(row) + 1, short_step=row[0] in SHORT_STEP_ROWS, device=0)
    assert counted == [(row[2], 0)]


# ------------------------------------------------------------------------------------ float64 evaluations
def formula_from_nonzeros(n, m, r, j, v, c, w):
    """The route's expressions in float64 from the nonzeros (r, j, v) alone, each with its magnitude (every term in
    absolute value): (G sampler, AW, AQc, sc) as (value, magnitude) pairs.  An honest float64 evaluation in any order
    is within c u M of the exact value for a small c; two of them within 2 c u M of each other."""
    sign = np.where(r == 0, -1.0, 1.0)
    u, um = np.zeros(m), np.zeros(m)
    np.add.at(u, j, v * w[r])
    np.add.at(um, j, np.abs(v * w[r]))
    h, hm = np.zeros(m), np.zeros(m)
    np.add.at(h, j, sign * v * c[r])
    np.add.at(hm, j, np.abs(v * c[r]))
    det, detm = w[0] * w[0] - w[1:] @ w[1:], w @ w
    wc, wcm = w @ c, np.abs(w) @ np.abs(c)
    z, zm = c[1:] @ c[1:] - c[0] * c[0], c @ c
    AW = (2 * u, 2 * um)
    AQc = (2 * (2 * wc * u + det * h), 2 * (2 * wcm * um + detm * hm))
    sc = (np.array([2 * wc, 2 * (2 * wc * wc + det * z)]), np.array([2 * wcm, 2 * (2 * wcm * wcm + detm * zm)]))
    return u, um, det, detm, AW, AQc, sc


def test_a_cone_over_4097_variables_against_float64():
    """The chunk edge of soc_sparse_gram is beyond what the longdouble reference does in seconds: the same formula in
    float64 numpy, the magnitude M built from absolute values with float64 BLAS, the bound 64 u M."""
    _, pattern, K, n, m = WIDE
    rng = np.random.default_rng(row_seed(WIDE))
    cn = km.make_cone("soc", n, m, None, 1e6, rng)
    A = cn["A"] = make_pattern(pattern, n, m, rng)
    k = km.build(SparseSocContext, [cn], [list(range(m))], m, device=0)
    assert k.count_sparse_soc() == 1
    k.set_W(0, cn["W"])
    k.assemble()
    G, AW, AQc, sc = k.constraint_schur(0)
    r, j = np.nonzero(A)
    u, um, det, detm, rAW, rAQc, rsc = formula_from_nonzeros(n, m, r, j, A[r, j], cn["c"], cn["W"])
    J = np.ones(n + 1)
    J[0] = -1.0
    H, Hm = A.T @ (J[:, None] * A), np.abs(A).T @ np.abs(A)
    Gr, Gm = 4 * np.outer(u, u) + 2 * det * H, 4 * np.outer(um, um) + 2 * detm * Hm
    bound = km.C_SCHUR * km.U
    assert np.all(np.abs(G - Gr) <= bound * Gm) and np.array_equal(G, G.T)
    assert G[m - 1, :].any() and G[COL_CHUNK - 1, :].any()  # both LDS chunks of a column carry entries
    for got, (val, mag) in ((AW, rAW), (AQc, rAQc), (sc, rsc)):
        assert np.all(np.abs(got - val) <= bound * mag)


# ------------------------------------------------------------------------------------ zeros, symmetry, same bits
def test_an_empty_variable_gets_exact_zeros_and_g_is_exactly_symmetric():
    row, cones, cliques, num_vars, y = row_problem("empty-column", 1e6)
    k = km.build(SparseSocContext, cones, cliques, num_vars, device=0)
    km.set_points(k, cones)
    k.assemble()
    m = row[4]
    for i in range(len(cones)):
        G, AW, AQc, _ = k.constraint_schur(i)
        assert not G[m - 1, :].any() and not G[:, m - 1].any() and AW[m - 1] == 0.0 and AQc[m - 1] == 0.0
        assert np.array_equal(G, G.T) and G[:m - 1, :m - 1].all()


@pytest.mark.parametrize("row_id", ["group-of-3", "block-513", "combine-1089"])
def test_g_is_exactly_symmetric(row_id):
    row, cones, cliques, num_vars, y = row_problem(row_id, 1e10)
    k = km.build(SparseSocContext, cones, cliques, num_vars, device=0)
    km.set_points(k, cones)
    k.assemble()
    for i in range(len(cones)):
        G = k.constraint_schur(i)[0]
        assert np.array_equal(G, G.T) and G.any()


def run_stages(cls, cones, cliques, num_vars, y, take="separate", build=km.build):
    """Every per-constraint output of the stages, as arrays, for bitwise comparisons."""
    k = build(cls, cones, cliques, num_vars, device=0)
    km.set_points(k, cones)
    out = {"sparse": k.count_sparse_soc(), "streamed": k.count_streamed_cones()}
    k.assemble()
    out["schur"] = [k.constraint_schur(i) for i in range(len(cones))]
    out["query"] = k.weighted_slack_eigenvalues(y, km.C_WEIGHT)
    if take == "separate":
        out["prepare"] = k.prepare_step(y, km.C_WEIGHT, 1.0)
        out["info"] = k.step_info()
        out["wsqrt"] = [k.get_W(i) for i in range(len(cones))]
        k.take_step(min(1.0, 2.0 / out["prepare"][1] ** 2), 1.0)
    else:
        n2, ninf, out["took"] = k.prepare_take_step(y, km.C_WEIGHT, 1.0)
        out["prepare"] = np.array([n2, ninf])
    out["W"] = [k.get_W(i) for i in range(len(cones))]
    return out


STAGE_KEYS = ("schur", "query", "prepare", "info", "wsqrt", "W")


def test_two_runs_give_the_same_bits():
    row, cones, cliques, num_vars, y = row_problem("group-of-3", 1e6)
    a = run_stages(SparseSocContext, cones, cliques, num_vars, y)
    b = run_stages(SparseSocContext, cones, cliques, num_vars, y)
    assert a["sparse"] == 3
    for key in STAGE_KEYS:
        assert ss.same_bits(a[key], b[key]), key


def test_the_sparse_and_the_streamed_route_agree():
    """The slack is the streamed route's chain without its zero terms and the step kernels are shared: everything
    behind the slack is equal bit for bit on identical W and y; only the Schur outputs differ, within the bound."""
    row = ss.ROWS[ss.ROW_IDS.index("image-edge")]
    assert row[3:5] == (319, 62)
    cones, cliques, num_vars = km.make_problem(row, 1e6, ss.row_seed(row))
    y = km.make_y(cones, cliques, num_vars, 5)
    sparse = run_stages(SparseSocContext, cones, cliques, num_vars, y)
    streamed = run_stages(StreamedContext, cones, cliques, num_vars, y)
    assert (sparse["sparse"], sparse["streamed"]) == (1, 0) and (streamed["sparse"], streamed["streamed"]) == (0, 1)
    for key in ("query", "prepare", "info", "wsqrt", "W"):
        assert ss.same_bits(sparse[key], streamed[key]), key
    low = np.tril(np.ones((62, 62), dtype=bool))
    for name, out, r in (("sparse", sparse, sparse_schur_reference(cones[0])), ("streamed", streamed, km.ref_schur(cones[0]))):
        g = r["g"]  # (1 for the expressions in w itself)
        G, AW, AQc, sc = out["schur"][0]
        km.within(G[low], r["G"][0][low], r["G"][1][low], km.C_SCHUR * g, f"G, {name}")
        km.within(AW, *r["AW"], km.C_SCHUR, f"AW, {name}")
        km.within(AQc, *r["AQc"], km.C_SCHUR * g, f"AQc, {name}")
        km.within(sc, *r["sc"], km.C_SCHUR * g, f"scalars, {name}")
    assert not ss.same_bits(sparse["schur"][0][0], streamed["schur"][0][0])  # (two formulas: the comparison is not empty)


def test_prepare_take_step_takes_sparse_cones():
    row, cones, cliques, num_vars, y = row_problem("group-of-3", "well")
    two = run_stages(SparseSocContext, cones, cliques, num_vars, y)
    one = run_stages(SparseSocContext, cones, cliques, num_vars, y, take="one-call")
    assert one["took"] == 1
    assert ss.same_bits(one["prepare"], two["prepare"]) and ss.same_bits(one["W"], two["W"])


# ------------------------------------------------------------------------------------ the CSR entry point
def build_csr(cls, cones, cliques, num_vars, device=0, rng=None):
    rng = rng or np.random.default_rng(12)
    k = cls(num_vars, device=device)
    for i, (cn, cl) in enumerate(zip(cones, cliques)):
        assert k.add_soc_csr(*ls.csr_of(cn["A"], rng), cn["c"], cl) == i
    k.initialize()
    return k


@pytest.mark.parametrize("row_id", ["empty-row", "group-of-3"])
def test_the_csr_entry_point_gives_the_bits_of_the_dense_one(row_id):
    """Shuffled columns and explicit zeros: the library sorts and drops them."""
    row, cones, cliques, num_vars, y = row_problem(row_id, 1e6)
    dense = run_stages(SparseSocContext, cones, cliques, num_vars, y)
    csr = run_stages(SparseSocContext, cones, cliques, num_vars, y, build=build_csr)
    assert dense["sparse"] == row[2] and csr["sparse"] == row[2]
    for key in STAGE_KEYS:
        assert ss.same_bits(dense[key], csr[key]), key


# (rowptr, col, val, c, message) for a cone with n = 1 (two rows) over ten variables
REFUSALS = [
    ([1, 2, 3], [0, 1, 2], [1.0, 1.0, 1.0], [1.0, 1.0], r"rowptr\[0\] is not 0"),
    ([0, 2, 1], [0, 1, 2], [1.0, 1.0, 1.0], [1.0, 1.0], r"rowptr decreases"),
    ([0, 1, 2], [0, 10], [1.0, 1.0], [1.0, 1.0], r"outside \[0, m\)"),
    ([0, 1, 2], [0, -1], [1.0, 1.0], [1.0, 1.0], r"outside \[0, m\)"),
    ([0, 3, 3], [4, 2, 4], [1.0, 1.0, 1.0], [1.0, 1.0], r"names a column twice"),
    (None, [0, 1], [1.0, 1.0], [1.0, 1.0], r"null"),
    ([0, 1, 2], None, [1.0, 1.0], [1.0, 1.0], r"null"),
    ([0, 1, 2], [0, 1], None, [1.0, 1.0], r"null"),
    ([0, 1, 2], [0, 1], [1.0, 1.0], None, r"null"),
]


def raw_add(k, n, m, rowptr, col, val, c):
    ip = lambda a: None if a is None else np.asarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))
    dp = lambda a: None if a is None else np.asarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    r = k.L.cxk_add_soc_csr(k.h, n, m, ip(rowptr), ip(col), dp(val), dp(c), None)
    return r, k.L.cxk_last_error(k.h).decode()


def check_refusal(k, rowptr, col, val, c, message):
    r, err = raw_add(k, 1, 10, rowptr, col, val, c)
    assert r == -1 and re.search(r"cxk_add_soc_csr.*" + message, err), err
    assert k.add_soc_csr([0, 1, 2], [0, 1], [1.0, 1.0], [1.0, 1.0]) == 0  # the context is still usable


@pytest.mark.parametrize("rowptr,col,val,c,message", REFUSALS)
def test_add_soc_csr_refuses_bad_input_by_name(rowptr, col, val, c, message):
    check_refusal(KktContext(10, device=0), rowptr, col, val, c, message)


def test_a_csr_cone_under_mode_0_is_refused_at_initialize():
    rng = np.random.default_rng(4)
    A = make_pattern("half", 19, 10, rng)
    c = np.r_[1.0, np.zeros(19)]
    k = KktContext(10, device=0)
    k.set_sparse_soc(0)
    assert k.add_soc_csr(*ls.csr_of(A, rng), c) == 0
    with pytest.raises(KktError, match=r"cxk_add_soc_csr.*sparse route.*cxk_set_sparse_soc"):
        k.initialize()
    k = KktContext(10, device=0)  # the device default is mode 0 too
    assert k.add_soc_csr(*ls.csr_of(A, rng), c) == 0
    with pytest.raises(KktError, match=r"cxk_add_soc_csr"):
        k.initialize()


# ------------------------------------------------------------------------------------ the switch
def one_cone(k, pattern="half", n=19, m=10):
    rng = np.random.default_rng(3)
    assert k.add_soc(make_pattern(pattern, n, m, rng), np.r_[1.0, np.zeros(n)]) == 0
    k.initialize()
    return k


def with_mode(mode, m=10, streamed=False):
    k = KktContext(m, device=0)
    if mode is not None:
        k.set_sparse_soc(mode)
    if streamed:  # (where the cone is beyond LDS on the dense side of the choice)
        k.set_streamed_cones()
    return k


def test_the_device_default_is_mode_0():
    assert one_cone(with_mode(None)).count_sparse_soc() == 0
    assert one_cone(with_mode(1), "dense").count_sparse_soc() == 1
    assert one_cone(with_mode(0)).count_sparse_soc() == 0


def test_the_environment_switch_equals_the_call(monkeypatch):
    monkeypatch.setenv("CXK_SPARSE_SOC", "1")
    assert one_cone(with_mode(None)).count_sparse_soc() == 1
    assert one_cone(with_mode(0)).count_sparse_soc() == 0  # an explicit call wins
    monkeypatch.setenv("CXK_SPARSE_SOC", "0")
    assert one_cone(with_mode(None)).count_sparse_soc() == 0
    assert one_cone(with_mode(1)).count_sparse_soc() == 1


def test_a_sparse_cone_needs_neither_the_streamed_switch_nor_lds_room():
    A, c = km.soc_data(319, 62)  # one past the LDS routes' admission edge
    k = KktContext(62, device=0)
    k.set_streamed_cones(False)
    k.set_sparse_soc(1)
    assert k.add_soc(A, c) == 0
    k.initialize()
    assert (k.count_sparse_soc(), k.count_streamed_cones()) == (1, 0)


def test_automatic_mode_takes_what_can_run_nowhere_else_and_what_pays(monkeypatch):
    """A cone added by its nonzeros is sparse whatever its shape; a dense-added one by kSparseSocMinRatio nnz <= len m
    above the floor on len m^2, the ratio movable through the environment."""
    rng = np.random.default_rng(6)
    k = with_mode(-1)
    assert k.add_soc_csr(*ls.csr_of(make_pattern("half", 19, 10, rng), rng), np.r_[1.0, np.zeros(19)]) == 0
    k.initialize()
    assert k.count_sparse_soc() == 1
    assert one_cone(with_mode(-1)).count_sparse_soc() == 0                  # 20 x 10: below the floor
    n, m = 2047, 64
    assert 20 * 10 * 10 < MIN_WORK <= (n + 1) * m * m and 1.0 < MIN_RATIO <= m / 3 < 22
    assert one_cone(with_mode(-1, m, True), "three", n, m).count_sparse_soc() == 1  # len m / nnz = 64 / 3
    assert one_cone(with_mode(-1, m, True), "dense", n, m).count_sparse_soc() == 0  # ratio 1 never moves
    monkeypatch.setenv("CXK_SPARSE_SOC_MIN_RATIO", "1")
    assert one_cone(with_mode(-1, m, True), "dense", n, m).count_sparse_soc() == 1
    monkeypatch.setenv("CXK_SPARSE_SOC_MIN_RATIO", "22")
    assert one_cone(with_mode(-1, m, True), "three", n, m).count_sparse_soc() == 0


def test_a_staged_cone_under_mode_0_keeps_its_bits():
    row = ("staged-edge", "soc", 5, 87, 27, None)  # km's last staged shape
    cones, cliques, num_vars = km.make_problem(row, 1e6, km.row_seed(row))
    y = km.make_y(cones, cliques, num_vars, 6)

    class Mode0(KktContext):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.set_sparse_soc(0)

    class Automatic(KktContext):  # (five cones of 88 x 27 are below the floor: automatic mode leaves them)
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.set_sparse_soc(-1)

    plain = run_stages(KktContext, cones, cliques, num_vars, y)
    for cls in (Mode0, Automatic):
        out = run_stages(cls, cones, cliques, num_vars, y)
        assert (out["sparse"], out["streamed"]) == (0, 0)
        for key in STAGE_KEYS:
            assert ss.same_bits(out[key], plain[key]), key


# ------------------------------------------------------------------------------------ a mixed context
def build_mixed(parts, with_big):
    """ss.build_mixed with the large cone added by its nonzeros under automatic mode, which leaves the small cone on
    its staged kernels."""
    big, small, (A, Cm, Wl) = parts
    k = KktContext(62, device=0)
    k.set_sparse_soc(-1)
    ids = {}
    if with_big:
        ids["big"] = k.add_soc_csr(*ls.csr_of(big["A"], np.random.default_rng(1)), big["c"], list(range(62)))
    ids["small"] = k.add_soc(small["A"], small["c"], list(range(10)))
    ids["lmi"] = k.add_lmi(A, Cm, list(range(10)))
    k.initialize()
    if with_big:
        k.set_W(ids["big"], big["W"])
    k.set_W(ids["small"], small["W"])
    k.set_W(ids["lmi"], Wl)
    return k, ids


@pytest.mark.parametrize("point", km.POINTS, ids=POINT_IDS)
def test_mixed_context(point):
    """One sparse cone, one staged second-order cone and one LMI over shared variables: the sparse cone against the
    reference, the other two bit for bit what they are without it (their kernels do not know who else is there)."""
    parts = ss.mixed_problem(point, 79)
    big, small, _ = parts
    big["A"] = big["A"] * (np.random.default_rng(80).random(big["A"].shape) < 0.1)
    k, ids = build_mixed(parts, True)
    alone, ids0 = build_mixed(parts, False)
    assert k.count_sparse_soc() == 1 and alone.count_sparse_soc() == 0 and k.count_streamed_cones() == 0
    y = np.random.default_rng(78).uniform(-1, 1, 62)
    y *= 0.5 / max(km.slack_scale(big, y), km.slack_scale(small, y[:10]))
    for ctx in (k, alone):
        ctx.assemble()
    G, AW, AQc, sc = k.constraint_schur(ids["big"])
    r = sparse_schur_reference(big)
    low = np.tril(np.ones_like(G, dtype=bool))
    km.within(G[low], r["G"][0][low], r["G"][1][low], km.C_SCHUR, "G of big")
    km.within(AW, *r["AW"], km.C_SCHUR, "AW of big")
    km.within(AQc, *r["AQc"], km.C_SCHUR, "AQc of big")
    km.within(sc, *r["sc"], km.C_SCHUR, "scalars of big")
    for name in ("small", "lmi"):
        assert ss.same_bits(k.constraint_schur(ids[name]), alone.constraint_schur(ids0[name])), name
    k.prepare_step(y, km.C_WEIGHT, 1.0)
    alone.prepare_step(y, km.C_WEIGHT, 1.0)
    info, info0 = k.step_info(), alone.step_info()
    p = km.ref_prepare(big, y)
    km.within(info[ids["big"], 0], *p["normsqrd"], km.C_PREPARE * p["g"], "normsqrd of big")
    km.within(info[ids["big"], 1], *p["norminfd"], km.C_PREPARE * p["g"], "norminfd of big")
    km.within(k.get_W(ids["big"]), *p["wsqrt"], km.C_PREPARE * p["g"], "w^1/2 of big")
    for name in ("small", "lmi"):
        assert ss.same_bits(info[ids[name]], info0[ids0[name]]), name
    k.take_step(0.5, 1.0)
    alone.take_step(0.5, 1.0)
    Wn, Wm = km.ref_take(big, y, 0.5)
    km.within(k.get_W(ids["big"]), Wn, Wm, km.C_TAKE * p["g"], "W after the step of big")
    for name in ("small", "lmi"):
        assert ss.same_bits(k.get_W(ids[name]), alone.get_W(ids0[name])), name


# ------------------------------------------------------------------------------------ size
def test_a_cone_whose_dense_matrix_is_beyond_the_int_range():
    """n = 600 000, m = 4000, two nonzeros per row: (n + 1) m = 2.4e9 entries, which both dense routes refuse.  By its
    nonzeros the cone finalizes, assembles and takes a step; AW, AQc, the scalars and 1000 entries of G against the
    formula evaluated from the nonzeros in float64 numpy (no dense matrix), within 64 u M."""
    n, m = 600_000, 4000
    assert (n + 1) * m > 2 ** 31
    rng = np.random.default_rng(2029)
    rows = n + 1
    j = np.stack([rng.integers(0, m // 2, rows), rng.integers(m // 2, m, rows)], axis=1)  # two distinct columns per row
    v = rng.uniform(-1, 1, (rows, 2))
    c = 0.2 * rng.uniform(-1, 1, rows)
    c[0] = 1.0
    w = np.r_[2.0, rng.uniform(-1, 1, n) / np.sqrt(n)]  # eigenvalues about 2 -+ 0.58
    k = KktContext(m, device=0)
    k.set_sparse_soc(-1)
    assert k.add_soc_csr(2 * np.arange(rows + 1), j.ravel(), v.ravel(), c) == 0
    k.initialize()
    assert (k.count_sparse_soc(), k.count_streamed_cones()) == (1, 0)
    assert k.sparse_soc_setup_ms() > 0.0  # (the constants were formed on the device, and clocked)
    k.set_W(0, w)
    k.assemble()
    G, AW, AQc, sc = k.constraint_schur(0)
    r = np.repeat(np.arange(rows), 2)
    u, um, det, detm, rAW, rAQc, rsc = formula_from_nonzeros(n, m, r, j.ravel(), v.ravel(), c, w)
    bound = km.C_SCHUR * km.U
    for got, (val, mag) in ((AW, rAW), (AQc, rAQc), (sc, rsc)):
        assert np.all(np.abs(got - val) <= bound * mag)
    # H[a, b] = sum over the rows holding both columns: a row's two columns are (low half, high half)
    H, Hm = {}, {}
    sign = np.where(np.arange(rows) == 0, -1.0, 1.0)
    for rr in range(rows):
        a, b = int(j[rr, 0]), int(j[rr, 1])
        for p_, q_, x in ((a, a, v[rr, 0] * v[rr, 0]), (b, b, v[rr, 1] * v[rr, 1]), (a, b, v[rr, 0] * v[rr, 1])):
            H[p_, q_] = H.get((p_, q_), 0.0) + sign[rr] * x
            Hm[p_, q_] = Hm.get((p_, q_), 0.0) + abs(x)
    pairs = [(int(j[rr, 0]), int(j[rr, 1])) for rr in rng.integers(0, rows, 600)]           # coupled entries
    pairs += [(int(a), int(a)) for a in rng.integers(0, m, 200)]                              # the diagonal
    pairs += [(int(a), int(b)) for a, b in zip(rng.integers(0, m // 2, 200), rng.integers(0, m // 2, 200)) if a != b]  # H = 0
    assert len(pairs) >= 990
    for a, b in pairs:
        val = 4 * u[a] * u[b] + 2 * det * H.get((a, b), 0.0)
        mag = 4 * um[a] * um[b] + 2 * detm * Hm.get((a, b), 0.0)
        assert abs(G[a, b] - val) <= bound * mag and G[a, b] == G[b, a], (a, b)
    y = rng.uniform(-1, 1, m) * 0.1
    n2, ninf = k.prepare_step(y, km.C_WEIGHT, 1.0)
    assert np.isfinite(n2) and np.isfinite(ninf) and ninf > 0
    k.take_step(min(1.0, 2.0 / ninf ** 2), 1.0)
    Wn = k.get_W(0)
    assert np.all(np.isfinite(Wn)) and Wn[0] > np.linalg.norm(Wn[1:]) and not np.array_equal(Wn, w)


# ------------------------------------------------------------------------------------ sharding
def test_sharded_direction_with_sparse_cones_equals_the_unsharded_one():
    """World 2 (the thread ranks of test_sharding.py) on a clique tree of half-empty cones, every one on the sparse
    route: one Newton iteration equals the single context's to that file's tolerance."""
    K, world = 40, 2
    prob = syn.soc_problem(K=K, dim=30, m=10, overlap=2, seed=21, tree=2)
    prob["A"] = prob["A"] * (np.random.default_rng(22).random(prob["A"].shape) < 0.5)
    W = syn.soc_scaling_points(K, 30, seed=23)
    single = syn.build(SparseSocContext, prob, "soc", device=0)
    assert single.count_sparse_soc() == K
    want = _newton_iteration(single, prob, W, False)

    def body(rank, allreduce):
        k = SparseSocContext(prob["num_vars"], device=0)
        for i, cl in enumerate(prob["cliques"]):
            assert k.add_soc(prob["A"][i], prob["c"][i], cl) == i
        k.set_shard(rank, world)
        k.initialize()
        k.comm_set_allreduce(allreduce)
        k.set_cost(prob["b"])
        out = _newton_iteration(k, prob, W, True)
        out["sparse"] = k.count_sparse_soc()
        return out

    outs = ThreadRanks(world).run(body)
    assert all(0 < out["sparse"] < K for out in outs) and sum(out["sparse"] for out in outs) >= K
    for out in outs:
        for key in ("y", "y2", "y3"):
            assert np.linalg.norm(out[key] - want[key]) <= 1e-10 * np.linalg.norm(want[key]), key
        assert np.allclose(out["eig"], want["eig"], rtol=1e-9, atol=0)
        assert np.allclose(out["info"], want["info"], rtol=1e-9, atol=0)
        for i, w in out["W"].items():
            assert np.linalg.norm(w - want["W"][i]) <= 1e-10 * np.linalg.norm(want["W"][i])
