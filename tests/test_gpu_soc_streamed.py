"""Second-order cones larger than LDS on the streamed kernels (kernels_soc_stream.hip.h), at the edges
of the new path, against the extended-precision reference of cone_reference.py.

The problems, the stages and the bounds are those of test_gpu_cone_kernel_matrix.py (make_problem /
run_rows / C_SCHUR, C_PREPARE, C_TAKE, imported): each row runs at the three scaling points through
assemble -> constraint_schur -> eigenvalue query -> PrepareStep -> TakeStep on a KktContext whose
constructor calls set_streamed_cones().  test_soc_streamed_reference.py runs the same rows on the
float64 oracle, which shows that correct float64 code meets the bounds at these lengths too.

Each row is the smallest shape at which its mechanism first engages; test_rows_sit_on_their_edges
recomputes every edge with the launch site's arithmetic (cone_route.h's three demands,
SocStreamSplits, the row tile of soc_stream_slack), so that a row cannot leave its edge unnoticed.
"""
import numpy as np
import pytest

import test_gpu_cone_kernel_matrix as km
from conex_amd import KktContext
from conex_amd.kkt import KktError
from conex_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ROW_TILE = 256        # kSocStreamRowTile
MIN_SPLIT_K = 1024    # kSocStreamMinSplitK
MFMA_TILE = 16        # v_mfma_f64_16x16x4_f64

# (id, kind, K, n, m, extra) as km.ROWS
ROWS = [
    ("image-edge", "soc", 1, 319, 62, None),      # len (m + 2) = 20480: first shape past the image rule
    ("take-edge", "soc", 1, 5104, 1, None),       # 4 len = 20420: first past soc_take_step's rule, m = 1
    ("prepare-edge", "soc", 1, 6805, 1, None),    # m + 3 len = 20419: first past soc_prepare's rule as well (6804: 20416, at it)
    ("group-of-3", "soc", 3, 400, 61, None),      # several cones in a group; m no multiple of the MFMA tile
    ("len-odd", "soc", 2, 1000, 33, None),        # len odd (the GEMM's general kernel); m one past two tiles
    ("split-k", "soc", 1, 2047, 17, None),        # len = 2 x 1024: the smallest len whose Gram product is split
    ("row-tile", "soc", 1, 1280, 15, None),       # len = 5 x 256 + 1: one row in the last tile of the slack
    ("short-step", "soc", 1, 1100, 18, None),     # y eight times the usual: TakeStep scales d (at all three points)
]
ROW_IDS = [r[0] for r in ROWS]
SHORT_STEP_ROWS = ("short-step",)


class StreamedContext(KktContext):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.set_streamed_cones()


def staged(n, m):
    """cone_route.h's three demands on a second-order cone, restated: True = it keeps the LDS kernels."""
    length = n + 1
    return (8 * length * (m + 2) <= km.K_LDS_LIMIT and 8 * 4 * length <= km.K_LDS_LIMIT
            and 8 * (m + 3 * length) <= km.K_LDS_LIMIT)


def gram_splits(n, m, count):
    """SocStreamSplits, restated."""
    tiles = ((m + 63) // 64) ** 2 * count
    return max(1, min((n + 1) // MIN_SPLIT_K, (512 + tiles - 1) // tiles))


def row_seed(row):
    return 4000 + km.row_seed(row)


def test_rows_sit_on_their_edges():
    shape = {r[0]: (r[2], r[3], r[4]) for r in ROWS}
    assert all(not staged(n, m) for _, n, m in shape.values())
    lim = km.K_LDS_LIMIT // 8  # 20 416 doubles
    _, n, m = shape["image-edge"]
    assert staged(n - 1, m) and (n + 1) * (m + 2) > lim >= n * (m + 2)
    _, n, m = shape["take-edge"]
    assert m == 1 and staged(n - 1, m) and 4 * (n + 1) > lim >= 4 * n and (n + 1) * (m + 2) <= lim
    _, n, m = shape["prepare-edge"]
    assert m == 1 and m + 3 * (n + 1) > lim >= m + 3 * n
    K, n, m = shape["group-of-3"]
    assert K > 1 and m % MFMA_TILE != 0
    K, n, m = shape["len-odd"]
    assert (n + 1) % 2 == 1 and m == 2 * MFMA_TILE + 1
    K, n, m = shape["split-k"]
    assert m == 17 and gram_splits(n, m, K) == 2 and gram_splits(n - 1, m, K) == 1
    assert all(gram_splits(r[3], r[4], r[2]) == 1 for r in ROWS if r[0] not in ("split-k", "take-edge", "prepare-edge"))
    K, n, m = shape["row-tile"]
    assert (n + 1) % ROW_TILE == 1 and n + 1 > ROW_TILE
    assert set(SHORT_STEP_ROWS) <= set(shape)


@pytest.mark.parametrize("point", km.POINTS, ids=lambda p: p if isinstance(p, str) else f"cond{p:.0e}")
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_streamed_kernel_matrix(row, point):
    cones, cliques, num_vars = km.make_problem(row, point, row_seed(row))
    counted = []

    class Counting(StreamedContext):
        def initialize(self):
            r = super().initialize()
            counted.append(self.count_streamed_cones())
            return r

    km.run_rows(Counting, cones, cliques, num_vars, row_seed(row) + 1, short_step=row[0] in SHORT_STEP_ROWS, device=0)
    assert counted == [row[2]]


# ------------------------------------------------------------------------------------ the switch
def test_without_the_switch_the_cone_is_refused_as_before():
    A, c = km.soc_data(319, 62)
    k = KktContext(62, device=0)
    assert k.add_soc(A, c) == 0
    with pytest.raises(KktError, match=r"LDS"):
        k.initialize()


def test_the_environment_switch_equals_the_call(monkeypatch):
    """CXK_STREAMED_CONES=1 is read by cxk_finalize (a host-only context chooses no kernels, so this is seen on the
    device only); an explicit call wins over it."""
    A, c = km.soc_data(319, 62)
    monkeypatch.setenv("CXK_STREAMED_CONES", "1")
    k = KktContext(62, device=0)
    assert k.add_soc(A, c) == 0
    k.initialize()
    assert k.count_streamed_cones() == 1
    k = KktContext(62, device=0)
    k.set_streamed_cones(False)
    assert k.add_soc(A, c) == 0
    with pytest.raises(KktError, match=r"LDS"):
        k.initialize()


def test_the_quadratic_cone_keeps_its_limits():
    A, c = km.soc_data(5103, 4)
    k = StreamedContext(4, device=0)
    assert k.add_quadratic(None, A, c) == 0
    with pytest.raises(KktError, match=r"quadratic cone.*LDS"):
        k.initialize()


def run_stages(cls, cones, cliques, num_vars, seed, take="separate"):
    """Every per-constraint output of the stages, as arrays, for bitwise comparisons."""
    k = km.build(cls, cones, cliques, num_vars, device=0)
    km.set_points(k, cones)
    y = km.make_y(cones, cliques, num_vars, seed)
    out = {"streamed": k.count_streamed_cones()}
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


def same_bits(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


def test_two_runs_give_the_same_bits():
    row = ROWS[ROW_IDS.index("split-k")]
    cones, cliques, num_vars = km.make_problem(row, 1e6, row_seed(row))
    a = run_stages(StreamedContext, cones, cliques, num_vars, 5)
    b = run_stages(StreamedContext, cones, cliques, num_vars, 5)
    assert a["streamed"] == 1
    for key in ("schur", "query", "prepare", "info", "wsqrt", "W"):
        assert same_bits(a[key], b[key]), key


def test_a_staged_cone_keeps_its_kernels_and_its_bits_with_the_switch_on():
    row = ("staged-edge", "soc", 5, 87, 27, None)  # km's last staged shape
    assert staged(87, 27)
    cones, cliques, num_vars = km.make_problem(row, 1e6, km.row_seed(row))
    off = run_stages(KktContext, cones, cliques, num_vars, 6)
    on = run_stages(StreamedContext, cones, cliques, num_vars, 6)
    assert on["streamed"] == 0 and off["streamed"] == 0
    for key in ("schur", "query", "prepare", "info", "wsqrt", "W"):
        assert same_bits(on[key], off[key]), key


def test_prepare_take_step_takes_streamed_cones():
    """The step length and c_weight are read on the device by the streamed kernels too: the one-call form
    takes the step (took = 1) and leaves the W of the two calls."""
    row = ROWS[ROW_IDS.index("image-edge")]
    cones, cliques, num_vars = km.make_problem(row, "well", row_seed(row))
    two = run_stages(StreamedContext, cones, cliques, num_vars, 7)
    one = run_stages(StreamedContext, cones, cliques, num_vars, 7, take="one-call")
    assert one["took"] == 1
    assert same_bits(one["prepare"], two["prepare"]) and same_bits(one["W"], two["W"])


# ------------------------------------------------------------------------------------ a mixed context
def mixed_problem(point, seed):
    """One streamed cone, one staged second-order cone (10, 10) and one LMI of order 6 over shared variables:
    the streamed cone over all 62, the other two over the first ten."""
    rng = np.random.default_rng(seed)
    big = km.make_cone("soc", 319, 62, None, point, rng)
    small = km.make_cone("soc", 10, 10, None, point, rng)
    lmi = syn.lmi_problem(K=1, n=6, m=10, branching=1, overlap=1, seed=seed)
    return big, small, (lmi["A"][0], lmi["C"][0], syn.scaling_points(1, 6, seed=seed + 1)[0])


def build_mixed(cls, parts, with_big):
    big, small, (A, Cm, Wl) = parts
    k = cls(62, device=0)
    ids = {}
    if with_big:
        ids["big"] = k.add_soc(big["A"], big["c"], list(range(62)))
    ids["small"] = k.add_soc(small["A"], small["c"], list(range(10)))
    ids["lmi"] = k.add_lmi(A, Cm, list(range(10)))
    k.initialize()
    if with_big:
        k.set_W(ids["big"], big["W"])
    k.set_W(ids["small"], small["W"])
    k.set_W(ids["lmi"], Wl)
    return k, ids


@pytest.mark.parametrize("point", km.POINTS, ids=lambda p: p if isinstance(p, str) else f"cond{p:.0e}")
def test_mixed_context(point):
    parts = mixed_problem(point, 77)
    big, small, _ = parts
    k, ids = build_mixed(StreamedContext, parts, True)
    alone, ids0 = build_mixed(StreamedContext, parts, False)
    assert k.count_streamed_cones() == 1 and alone.count_streamed_cones() == 0
    y = np.random.default_rng(78).uniform(-1, 1, 62)
    y *= 0.5 / max(km.slack_scale(big, y), km.slack_scale(small, y[:10]))
    for ctx in (k, alone):
        ctx.assemble()
    # the two second-order cones against the reference, the LMI and the staged cone against the context without
    # the streamed cone, bit for bit (their kernels do not know who else is there)
    for name, cn, z in (("big", big, y), ("small", small, y[:10])):
        G, AW, AQc, sc = k.constraint_schur(ids[name])
        r = km.ref_schur(cn)
        low = np.tril(np.ones_like(G, dtype=bool))
        km.within(G[low], r["G"][0][low], r["G"][1][low], km.C_SCHUR * r["g"], f"G of {name}")
        km.within(AW, *r["AW"], km.C_SCHUR, f"AW of {name}")
        km.within(AQc, *r["AQc"], km.C_SCHUR * r["g"], f"AQc of {name}")
        km.within(sc, *r["sc"], km.C_SCHUR * r["g"], f"scalars of {name}")
    for name in ("small", "lmi"):
        assert same_bits(k.constraint_schur(ids[name]), alone.constraint_schur(ids0[name])), name
    k.prepare_step(y, km.C_WEIGHT, 1.0)
    alone.prepare_step(y, km.C_WEIGHT, 1.0)
    info, info0 = k.step_info(), alone.step_info()
    p = {"big": km.ref_prepare(big, y), "small": km.ref_prepare(small, y[:10])}
    for name in ("big", "small"):
        i, g = ids[name], p[name]["g"]
        km.within(info[i, 0], *p[name]["normsqrd"], km.C_PREPARE * g, f"normsqrd of {name}")
        km.within(info[i, 1], *p[name]["norminfd"], km.C_PREPARE * g, f"norminfd of {name}")
        km.within(k.get_W(i), *p[name]["wsqrt"], km.C_PREPARE * g, f"w^1/2 of {name}")
    for name in ("small", "lmi"):
        assert same_bits(info[ids[name]], info0[ids0[name]]), name
    step = 0.5
    k.take_step(step, 1.0)
    alone.take_step(step, 1.0)
    for name, cn, z in (("big", big, y), ("small", small, y[:10])):
        Wn, Wm = km.ref_take(cn, z, step)
        km.within(k.get_W(ids[name]), Wn, Wm, km.C_TAKE * p[name]["g"], f"W after the step of {name}")
    for name in ("small", "lmi"):
        assert same_bits(k.get_W(ids[name]), alone.get_W(ids0[name])), name
