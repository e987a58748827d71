"""Quadratic cones on the streamed kernels (kernels_quad_stream.hip.h), at the edges of the new path, against the
extended-precision reference of cone_reference.py.

The problems, the stages and the bounds are those of test_gpu_cone_kernel_matrix.py (make_problem / run_rows /
C_SCHUR, C_PREPARE, C_TAKE, imported unchanged): each row runs at the three scaling points through assemble ->
constraint_schur -> eigenvalue query -> PrepareStep -> TakeStep on a KktContext whose constructor calls
set_streamed_quadratic(1).  test_quad_streamed_reference.py runs the same rows on the float64 oracle, which shows
that correct float64 code meets the bounds at these sizes too.

test_rows_sit_on_their_edges recomputes every edge with the launch site's arithmetic (cone_route.h's three
demands, QuadStreamSplits, the row tile and the x chunk of quad_stream_qmv, the 256-entry blocks of the Schur
block), so that a row cannot leave its edge unnoticed.
"""
import numpy as np
import pytest

import test_gpu_cone_kernel_matrix as km
import test_gpu_soc_streamed as soc
from conex_amd import KktContext
from conex_amd.kkt import KktError
from conex_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ROW_TILE = 256     # kQuadStreamRowTile
X_CHUNK = 64       # kQuadStreamXChunk
MIN_SPLIT = 64     # kQuadStreamMinSplit
BLOCK = 256        # kQuadStreamBlock: entries of G per workgroup of quad_stream_schur_finish
HUGE = str(1 << 60)

# (id, kind, K, n, m, extra) as km.ROWS
ROWS = [
    ("min-q", "quad", 1, 1, 1, "Q"),
    ("min-noq", "quad", 1, 1, 1, None),
    ("row-tile", "quad", 1, 257, 3, "Q"),         # one row past a 256-row tile; y eight times the usual (short step)
    ("group-of-3", "quad", 3, 300, 5, "Q"),       # several cones in a group
    ("m65", "quad", 2, 64, 65, "Q"),              # m * m = 4225: seventeen blocks of the Schur block; n one chunk, one split
    ("square", "quad", 1, 320, 320, "Q"),
    ("tiles-5", "quad", 1, 1025, 2, "Q"),         # five row tiles, one row in the last
    ("prepare-edge", "quad", 1, 5103, 4, None),   # m + 4 len = 20420 doubles: first past quad_prepare's demand
    ("noq-6804", "quad", 1, 6804, 1, None),
    ("first-split", "quad", 1, 128, 3, "Q"),      # n = 2 x 64: the smallest order whose columns are split
    ("partial-chunk", "quad", 1, 127, 3, "Q"),    # one split of 64 + 63 columns: a partial last chunk of x
]
ROW_IDS = [r[0] for r in ROWS]
SHORT_STEP_ROWS = ("row-tile",)


class StreamedQuad(KktContext):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.set_streamed_quadratic(1)


class AutomaticQuad(KktContext):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.set_streamed_quadratic(-1)


def lds_route(n, m):
    """cone_route.h's three demands on a quadratic cone, restated: True = the LDS kernels can hold it."""
    return (8 * (m + 4 * (n + 1)) <= km.K_LDS_LIMIT and 8 * (2 * n + m + 4) <= km.K_LDS_LIMIT
            and 8 * 3 * (n + 1) <= km.K_LDS_LIMIT)


def column_splits(n, count):
    """QuadStreamSplits, restated."""
    tiles = ((n + ROW_TILE - 1) // ROW_TILE) * count
    return max(1, min(n // MIN_SPLIT, (512 + tiles - 1) // tiles))


def split_chunks(n, count):
    """The chunk lengths of every split of quad_stream_qmv, restated."""
    splits = column_splits(n, count)
    per = (n + splits - 1) // splits
    out = []
    for s in range(splits):
        j0 = min(n, s * per)
        j1 = min(n, j0 + per)
        out.append([min(X_CHUNK, j1 - c0) for c0 in range(j0, j1, X_CHUNK)])
    return out


def row_seed(row):
    return 7000 + km.row_seed(row)


def test_rows_sit_on_their_edges():
    shape = {r[0]: (r[2], r[3], r[4], r[5]) for r in ROWS}
    lim = km.K_LDS_LIMIT // 8  # 20 416 doubles
    K, n, m, _ = shape["prepare-edge"]
    assert not lds_route(n, m) and lds_route(n - 1, m) and m + 4 * (n + 1) > lim >= m + 4 * n
    K, n, m, _ = shape["noq-6804"]
    assert not lds_route(n, m)
    assert all(lds_route(r[3], r[4]) for r in ROWS if r[0] not in ("prepare-edge", "noq-6804"))
    K, n, m, _ = shape["row-tile"]
    assert n % ROW_TILE == 1 and n > ROW_TILE
    K, n, m, _ = shape["tiles-5"]
    assert n % ROW_TILE == 1 and (n + ROW_TILE - 1) // ROW_TILE == 5
    K, n, m, q = shape["first-split"]
    assert q == "Q" and column_splits(n, K) == 2 and column_splits(n - 1, K) == 1
    assert all(len(c) == 1 and c[0] == X_CHUNK for c in split_chunks(n, K))
    K, n, m, q = shape["partial-chunk"]
    assert q == "Q" and column_splits(n, K) == 1 and split_chunks(n, K) == [[X_CHUNK, X_CHUNK - 1]]
    K, n, m, _ = shape["m65"]
    assert (m * m + BLOCK - 1) // BLOCK == 17 and m * m % BLOCK != 0 and split_chunks(n, K) == [[X_CHUNK]]
    K, n, m, _ = shape["group-of-3"]
    assert K > 1 and column_splits(n, K) == 4 and any(c[-1] < X_CHUNK for c in split_chunks(n, K))
    K, n, m, _ = shape["row-tile"]
    assert column_splits(n, K) == 4 and split_chunks(n, K)[0] == [X_CHUNK, 1]
    assert set(SHORT_STEP_ROWS) <= set(shape)


@pytest.mark.parametrize("point", km.POINTS, ids=lambda p: p if isinstance(p, str) else f"cond{p:.0e}")
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_streamed_quadratic_kernel_matrix(row, point):
    cones, cliques, num_vars = km.make_problem(row, point, row_seed(row))
    counted = []

    class Counting(StreamedQuad):
        def initialize(self):
            r = super().initialize()
            counted.append(self.count_streamed_quadratic())
            return r

    km.run_rows(Counting, cones, cliques, num_vars, row_seed(row) + 1, short_step=row[0] in SHORT_STEP_ROWS, device=0)
    assert counted == [row[2]]


# ------------------------------------------------------------------------------------ the switch
def beyond_lds(cls=KktContext):
    A, c = km.soc_data(5103, 4)
    k = cls(4, device=0)
    assert k.add_quadratic(None, A, c) == 0
    return k


def test_without_the_switch_the_cone_is_refused_as_before():
    with pytest.raises(KktError, match=r"quadratic cone.*LDS"):
        beyond_lds().initialize()


def test_the_environment_switch_equals_the_call(monkeypatch):
    monkeypatch.setenv("CXK_STREAMED_QUADRATIC", "1")
    k = beyond_lds()
    k.initialize()
    assert k.count_streamed_quadratic() == 1 and k.count_streamed_cones() == 0
    k = beyond_lds()
    k.set_streamed_quadratic(0)  # an explicit call wins over the environment
    with pytest.raises(KktError, match=r"quadratic cone.*LDS"):
        k.initialize()


def test_automatic_mode_with_a_huge_threshold_takes_only_the_cone_beyond_lds(monkeypatch):
    monkeypatch.setenv("CXK_STREAMED_QUADRATIC_MIN_WORK", HUGE)
    rng = np.random.default_rng(3)
    A, c = km.soc_data(5103, 4)
    small = km.make_cone("quad", 5, 4, "Q", "well", rng)
    k = AutomaticQuad(4, device=0)
    assert k.add_quadratic(None, A, c) == 0
    assert k.add_quadratic(small["Q"], small["A"], small["c"]) == 1
    k.initialize()
    assert k.count_streamed_quadratic() == 1


def test_streamed_second_order_cones_alone_still_refuse_a_quadratic_cone():
    with pytest.raises(KktError, match=r"quadratic cone.*LDS"):
        beyond_lds(soc.StreamedContext).initialize()


# ------------------------------------------------------------------------------------ bits
def run_stages(cls, cones, cliques, num_vars, seed, take="separate"):
    out = soc.run_stages(cls, cones, cliques, num_vars, seed, take)
    return out


def count_of(cls, cones, cliques, num_vars):
    return km.build(cls, cones, cliques, num_vars, device=0).count_streamed_quadratic()


STAGE_KEYS = ("schur", "query", "prepare", "info", "wsqrt", "W")


def test_two_runs_give_the_same_bits():
    row = ROWS[ROW_IDS.index("row-tile")]  # four column splits
    cones, cliques, num_vars = km.make_problem(row, 1e6, row_seed(row))
    assert count_of(StreamedQuad, cones, cliques, num_vars) == 1
    a = run_stages(StreamedQuad, cones, cliques, num_vars, 5)
    b = run_stages(StreamedQuad, cones, cliques, num_vars, 5)
    for key in STAGE_KEYS:
        assert soc.same_bits(a[key], b[key]), key


def test_an_lds_cone_keeps_its_kernels_and_its_bits_in_automatic_mode(monkeypatch):
    monkeypatch.setenv("CXK_STREAMED_QUADRATIC_MIN_WORK", HUGE)
    row = ("quad-q", "quad", 3, 5, 4, "Q")
    cones, cliques, num_vars = km.make_problem(row, 1e6, km.row_seed(row))
    assert count_of(AutomaticQuad, cones, cliques, num_vars) == 0
    off = run_stages(KktContext, cones, cliques, num_vars, 6)
    on = run_stages(AutomaticQuad, cones, cliques, num_vars, 6)
    for key in STAGE_KEYS:
        assert soc.same_bits(on[key], off[key]), key


def test_prepare_take_step_takes_streamed_quadratic_cones():
    """The step length and c_weight are read on the device by the streamed kernels too: the one-call form takes the
    step (took = 1) and leaves the W of the two calls."""
    row = ROWS[ROW_IDS.index("group-of-3")]
    cones, cliques, num_vars = km.make_problem(row, "well", row_seed(row))
    two = run_stages(StreamedQuad, cones, cliques, num_vars, 7)
    one = run_stages(StreamedQuad, cones, cliques, num_vars, 7, take="one-call")
    assert one["took"] == 1
    assert soc.same_bits(one["prepare"], two["prepare"]) and soc.same_bits(one["W"], two["W"])


# ------------------------------------------------------------------------------------ a mixed context
MIXED_MIN_WORK = 10000  # between the two quadratic cones below: 128 * 128 + 129 * 62 and 5 * 5 + 6 * 10 doubles per pass


class MixedContext(KktContext):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.set_streamed_cones()
        self.set_streamed_quadratic(-1)


def mixed_problem(point, seed):
    """One streamed quadratic cone with Q (128, 62), one LDS-route quadratic cone (5, 10), one streamed second-order
    cone (319, 62) and one LMI of order 6 over shared variables: the two big cones over all 62, the others over the
    first ten."""
    rng = np.random.default_rng(seed)
    big = km.make_cone("quad", 128, 62, "Q", point, rng)
    small = km.make_cone("quad", 5, 10, "Q", point, rng)
    cone = km.make_cone("soc", 319, 62, None, point, rng)
    lmi = syn.lmi_problem(K=1, n=6, m=10, branching=1, overlap=1, seed=seed)
    return big, small, cone, (lmi["A"][0], lmi["C"][0], syn.scaling_points(1, 6, seed=seed + 1)[0])


def build_mixed(parts, with_big):
    big, small, cone, (A, Cm, Wl) = parts
    k = MixedContext(62, device=0)
    ids = {}
    if with_big:
        ids["big"] = k.add_quadratic(big["Q"], big["A"], big["c"], list(range(62)))
    ids["small"] = k.add_quadratic(small["Q"], small["A"], small["c"], list(range(10)))
    ids["cone"] = k.add_soc(cone["A"], cone["c"], list(range(62)))
    ids["lmi"] = k.add_lmi(A, Cm, list(range(10)))
    k.initialize()
    if with_big:
        k.set_W(ids["big"], big["W"])
    k.set_W(ids["small"], small["W"])
    k.set_W(ids["cone"], cone["W"])
    k.set_W(ids["lmi"], Wl)
    return k, ids


@pytest.mark.parametrize("point", km.POINTS, ids=lambda p: p if isinstance(p, str) else f"cond{p:.0e}")
def test_mixed_context(point, monkeypatch):
    monkeypatch.setenv("CXK_STREAMED_QUADRATIC_MIN_WORK", str(MIXED_MIN_WORK))
    assert 5 * 5 + 6 * 10 < MIXED_MIN_WORK <= 128 * 128 + 129 * 62
    parts = mixed_problem(point, 79)
    big, small, cone, _ = parts
    k, ids = build_mixed(parts, True)
    alone, ids0 = build_mixed(parts, False)
    assert k.count_streamed_cones() == 1 and k.count_streamed_quadratic() == 1
    assert alone.count_streamed_cones() == 1 and alone.count_streamed_quadratic() == 0
    y = np.random.default_rng(80).uniform(-1, 1, 62)
    y *= 0.5 / max(km.slack_scale(big, y), km.slack_scale(cone, y), km.slack_scale(small, y[:10]))
    for ctx in (k, alone):
        ctx.assemble()
    # the streamed cones against the reference; the LDS-route quadratic cone and the LMI against the context without
    # the streamed quadratic cone, bit for bit (their kernels do not know who else is there)
    streamed = (("big", big, y), ("cone", cone, y))
    for name, cn, z in streamed:
        G, AW, AQc, sc = k.constraint_schur(ids[name])
        r = km.ref_schur(cn)
        low = np.tril(np.ones_like(G, dtype=bool))
        km.within(G[low], r["G"][0][low], r["G"][1][low], km.C_SCHUR * r["g"], f"G of {name}")
        km.within(AW, *r["AW"], km.C_SCHUR, f"AW of {name}")
        km.within(AQc, *r["AQc"], km.C_SCHUR * r["g"], f"AQc of {name}")
        km.within(sc, *r["sc"], km.C_SCHUR * r["g"], f"scalars of {name}")
    for name in ("small", "lmi"):
        assert soc.same_bits(k.constraint_schur(ids[name]), alone.constraint_schur(ids0[name])), name
    k.prepare_step(y, km.C_WEIGHT, 1.0)
    alone.prepare_step(y, km.C_WEIGHT, 1.0)
    info, info0 = k.step_info(), alone.step_info()
    p = {name: km.ref_prepare(cn, z) for name, cn, z in streamed}
    for name, cn, z in streamed:
        i, g = ids[name], p[name]["g"]
        km.within(info[i, 0], *p[name]["normsqrd"], km.C_PREPARE * g, f"normsqrd of {name}")
        km.within(info[i, 1], *p[name]["norminfd"], km.C_PREPARE * g, f"norminfd of {name}")
        km.within(k.get_W(i), *p[name]["wsqrt"], km.C_PREPARE * g, f"w^1/2 of {name}")
    for name in ("small", "lmi"):
        assert soc.same_bits(info[ids[name]], info0[ids0[name]]), name
    step = 0.5
    k.take_step(step, 1.0)
    alone.take_step(step, 1.0)
    for name, cn, z in streamed:
        Wn, Wm = km.ref_take(cn, z, step)
        km.within(k.get_W(ids[name]), Wn, Wm, km.C_TAKE * p[name]["g"], f"W after the step of {name}")
    for name in ("small", "lmi"):
        assert soc.same_bits(k.get_W(ids[name]), alone.get_W(ids0[name])), name
