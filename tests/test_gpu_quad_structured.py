"""Quadratic cones whose Q = S + F diag(sigma) F' is given by its parts (cxk_add_quadratic_structured,
kernels_quad_structured.hip.h), at the edges of the new kernels, against the extended-precision reference of
cone_reference.py.

The stages and the bounds are those of test_gpu_cone_kernel_matrix.py (run_rows / C_SCHUR, C_PREPARE, C_TAKE, imported
unchanged); the rows, their data and the context class are quad_structured_cases.py's.  Each row runs at the three
scaling points on a StructuredQuad context, whose add_quadratic hands the parts to add_quadratic_structured: the
reference sees the expansion of Q in longdouble, the device never sees it.  test_quad_structured_reference.py runs the
same rows on the float64 oracle with the expansion rounded to float64, which shows that correct float64 code meets the
bounds at these shapes.

Beyond the dense form (n = 50 000 > 46 340) the reference is quad_structured_cases.quad_schur_op, cone_reference's
quad_schur restated on the operators S x + F (sigma o F' x); test_quad_structured_reference.py pins it to quad_schur on
every row small enough.
"""
import numpy as np
import pytest

import cone_reference as ref
import quad_structured_cases as qc
import test_gpu_cone_kernel_matrix as km
import test_gpu_soc_streamed as soc
from conex_amd import KktContext
from conex_amd.kkt import KktError
from conex_amd import synthetic as syn

pytestmark = pytest.mark.gpu

POINT_IDS = [p if isinstance(p, str) else f"cond{p:.0e}" for p in km.POINTS]
STAGE_KEYS = ("schur", "query", "prepare", "info", "wsqrt", "W")


def counting(counted):
    class Counting(qc.StructuredQuad):
        def initialize(self):
            r = super().initialize()
            counted.append((self.count_structured_quadratic(), self.count_streamed_quadratic()))
            return r

    return Counting


def test_rows_sit_on_their_edges():
    qc.test_rows_sit_on_their_edges()


@pytest.mark.parametrize("point", km.POINTS, ids=POINT_IDS)
@pytest.mark.parametrize("row", [r for r in qc.ROWS if r[0] != "arrow"], ids=[i for i in qc.ROW_IDS if i != "arrow"])
def test_structured_quadratic_kernel_matrix(row, point):
    cones, cliques, num_vars = qc.make_problem(row, point)
    counted = []
    km.run_rows(counting(counted), cones, cliques, num_vars, qc.row_seed(row) + 1, short_step=row[0] in qc.SHORT_STEP_ROWS, device=0)
    assert counted == [(row[1], row[1])]


@pytest.mark.parametrize("lanes", qc.LANES)
@pytest.mark.parametrize("point", km.POINTS, ids=POINT_IDS)
def test_the_arrow_under_each_lane_count(point, lanes, monkeypatch):
    """One row of 300 nonzeros beside rows of 2: on one lane a long chain, on 8 and 64 lanes the strided chains and the
    butterfly, with most lanes of the short rows idle."""
    monkeypatch.setenv("CXK_QUAD_CSR_LANES", str(lanes))
    row = qc.ROWS[qc.ROW_IDS.index("arrow")]
    cones, cliques, num_vars = qc.make_problem(row, point)
    counted = []
    km.run_rows(counting(counted), cones, cliques, num_vars, qc.row_seed(row) + 1, device=0)
    assert counted == [(1, 1)]


# ------------------------------------------------------------------------------------ beyond the dense form
BIG_N, BIG_M = 50_000, 3


def big_problem():
    """n = 50 000 > 46 340 (n^2 past the int range), m = 3, tridiagonal S plus rank 2, W well inside the cone."""
    rng = np.random.default_rng(50_000)
    parts = dict(S=qc.banded(rng, BIG_N, 1), F=qc.make_f(BIG_N, 2, rng), sigma=rng.uniform(0.5, 1.5, 2))
    c = 0.2 * rng.uniform(-1, 1, BIG_N + 1)
    c[0] = 1.0
    A = rng.uniform(-1, 1, (BIG_N + 1, BIG_M))
    w1 = rng.uniform(-0.3, 0.3, BIG_N)
    k = float(np.sqrt(w1 @ qc.apply_q(parts, w1)))
    W = np.r_[k + rng.uniform(0.5, 1.5), w1]
    return parts, A, c, W / (W[0] + k)


def in_cone(parts, W):
    W = ref.ld(W)
    return bool(np.all(np.isfinite(W)) and W[0] > 0 and W[0] * W[0] > W[1:] @ qc.apply_q(parts, W[1:]))


def test_an_order_beyond_the_dense_form():
    assert BIG_N * BIG_N > 2 ** 31 - 1
    parts, A, c, W = big_problem()
    k = KktContext(BIG_M, device=0)
    assert k.add_quadratic_structured(parts["S"], parts["F"], parts["sigma"], A, c) == 0
    k.initialize()
    assert k.count_structured_quadratic() == 1 and k.count_streamed_quadratic() == 1
    k.set_W(0, W)
    k.assemble()
    G, AW, AQc, sc = k.constraint_schur(0)
    r = qc.quad_schur_op(A, c, W, parts)
    low = np.tril(np.ones_like(G, dtype=bool))
    km.within(G[low], r["G"][0][low], r["G"][1][low], km.C_SCHUR, "G")
    km.within(AW, *r["AW"], km.C_SCHUR, "AW")
    km.within(AQc, *r["AQc"], km.C_SCHUR, "AQc")
    km.within(sc, *r["sc"], km.C_SCHUR, "scalars")
    y = np.random.default_rng(1).uniform(-1, 1, BIG_M)
    y *= 0.5 / float(np.max(np.abs(A) @ np.abs(y)))
    info = k.prepare_step(y, km.C_WEIGHT, 1.0)
    assert np.all(np.isfinite(info)) and info[1] > 0
    k.take_step(min(1.0, 2.0 / info[1] ** 2), 1.0)
    assert in_cone(parts, k.get_W(0))


# ------------------------------------------------------------------------------------ bits
def run_stages(cones, cliques, num_vars, seed, take="separate"):
    return soc.run_stages(qc.StructuredQuad, cones, cliques, num_vars, seed, take)


@pytest.mark.parametrize("row_id,lanes", [("row-tile", None), ("arrow", 64)])
def test_two_runs_give_the_same_bits(row_id, lanes, monkeypatch):
    if lanes:
        monkeypatch.setenv("CXK_QUAD_CSR_LANES", str(lanes))
    row = qc.ROWS[qc.ROW_IDS.index(row_id)]
    cones, cliques, num_vars = qc.make_problem(row, 1e6)
    a = run_stages(cones, cliques, num_vars, 5)
    b = run_stages(cones, cliques, num_vars, 5)
    for key in STAGE_KEYS:
        assert soc.same_bits(a[key], b[key]), key


def test_prepare_take_step_in_one_call_equals_the_two_calls():
    row = qc.ROWS[qc.ROW_IDS.index("group-of-3")]
    cones, cliques, num_vars = qc.make_problem(row, "well")
    two = run_stages(cones, cliques, num_vars, 7)
    one = run_stages(cones, cliques, num_vars, 7, take="one-call")
    assert one["took"] == 1
    assert soc.same_bits(one["prepare"], two["prepare"]) and soc.same_bits(one["W"], two["W"])


# ------------------------------------------------------------------------------------ the switch
def test_streamed_mode_zero_does_not_refuse_a_structured_cone_and_still_refuses_a_dense_one_beyond_lds():
    row = qc.ROWS[qc.ROW_IDS.index("row-tile")]
    cones, cliques, num_vars = qc.make_problem(row, "well")
    cn = cones[0]
    k = qc.StructuredQuad(num_vars, device=0)
    k.set_streamed_quadratic(0)
    assert k.add_quadratic(cn["Q"], cn["A"], cn["c"], cliques[0]) == 0
    k.initialize()
    assert k.count_structured_quadratic() == 1 and k.count_streamed_quadratic() == 1
    k.set_W(0, cn["W"])
    k.assemble()
    G, AW, AQc, sc = k.constraint_schur(0)
    r = km.ref_schur(cn)
    km.within(AW, *r["AW"], km.C_SCHUR, "AW")
    # the same mode with a structured cone aboard: a dense cone beyond LDS is refused with today's message
    A, c = km.soc_data(5103, 4)
    k = qc.StructuredQuad(4, device=0)
    k.set_streamed_quadratic(0)
    small = qc.make_cone(5, 4, qc.make_parts("tridiagonal", 5, 1, 0, np.random.default_rng(2)), "well", np.random.default_rng(3))
    assert k.add_quadratic(small["Q"], small["A"], small["c"]) == 0
    assert k.add_quadratic(None, A, c) == 1
    with pytest.raises(KktError, match=r"quadratic cone.*LDS"):
        k.initialize()


# ------------------------------------------------------------------------------------ a mixed context
MIXED_MIN_WORK = 10000  # between the two dense quadratic cones below, as test_gpu_quad_streamed.MIXED_MIN_WORK


class MixedContext(qc.StructuredQuad):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.set_streamed_quadratic(-1)


def mixed_problem(point, seed):
    """One structured cone (300, 62: tridiagonal plus rank 4), one dense-Q streamed cone (128, 62), one LDS-route
    quadratic cone (5, 10) and one LMI of order 6 over shared variables: the two big cones over all 62, the others over
    the first ten."""
    rng = np.random.default_rng(seed)
    st = qc.make_cone(300, 62, qc.make_parts("tridiagonal", 300, 4, 0, rng), point, rng)
    big = km.make_cone("quad", 128, 62, "Q", point, rng)
    small = km.make_cone("quad", 5, 10, "Q", point, rng)
    lmi = syn.lmi_problem(K=1, n=6, m=10, branching=1, overlap=1, seed=seed)
    return st, big, small, (lmi["A"][0], lmi["C"][0], syn.scaling_points(1, 6, seed=seed + 1)[0])


def build_mixed(parts, with_structured):
    st, big, small, (A, Cm, Wl) = parts
    k = MixedContext(62, device=0)
    ids = {}
    if with_structured:
        ids["st"] = k.add_quadratic(st["Q"], st["A"], st["c"], list(range(62)))
    ids["big"] = k.add_quadratic(big["Q"], big["A"], big["c"], list(range(62)))
    ids["small"] = k.add_quadratic(small["Q"], small["A"], small["c"], list(range(10)))
    ids["lmi"] = k.add_lmi(A, Cm, list(range(10)))
    k.initialize()
    if with_structured:
        k.set_W(ids["st"], st["W"])
    k.set_W(ids["big"], big["W"])
    k.set_W(ids["small"], small["W"])
    k.set_W(ids["lmi"], Wl)
    return k, ids


@pytest.mark.parametrize("point", km.POINTS, ids=POINT_IDS)
def test_mixed_context(point, monkeypatch):
    monkeypatch.setenv("CXK_STREAMED_QUADRATIC_MIN_WORK", str(MIXED_MIN_WORK))
    assert 5 * 5 + 6 * 10 < MIXED_MIN_WORK <= 128 * 128 + 129 * 62
    parts = mixed_problem(point, 83)
    st, big, small, _ = parts
    k, ids = build_mixed(parts, True)
    alone, ids0 = build_mixed(parts, False)
    assert k.count_structured_quadratic() == 1 and k.count_streamed_quadratic() == 2
    assert alone.count_structured_quadratic() == 0 and alone.count_streamed_quadratic() == 1
    y = np.random.default_rng(84).uniform(-1, 1, 62)
    y *= 0.5 / max(km.slack_scale(st, y), km.slack_scale(big, y), km.slack_scale(small, y[:10]))
    others = ("big", "small", "lmi")
    for ctx in (k, alone):
        ctx.assemble()
    G, AW, AQc, sc = k.constraint_schur(ids["st"])
    r = km.ref_schur(st)
    low = np.tril(np.ones_like(G, dtype=bool))
    km.within(G[low], r["G"][0][low], r["G"][1][low], km.C_SCHUR * r["g"], "G of the structured cone")
    km.within(AW, *r["AW"], km.C_SCHUR, "AW of the structured cone")
    km.within(AQc, *r["AQc"], km.C_SCHUR * r["g"], "AQc of the structured cone")
    km.within(sc, *r["sc"], km.C_SCHUR * r["g"], "scalars of the structured cone")
    for name in others:
        assert soc.same_bits(k.constraint_schur(ids[name]), alone.constraint_schur(ids0[name])), name
    k.prepare_step(y, km.C_WEIGHT, 1.0)
    alone.prepare_step(y, km.C_WEIGHT, 1.0)
    info, info0 = k.step_info(), alone.step_info()
    p = km.ref_prepare(st, y)
    i, g = ids["st"], p["g"]
    km.within(info[i, 0], *p["normsqrd"], km.C_PREPARE * g, "normsqrd of the structured cone")
    km.within(info[i, 1], *p["norminfd"], km.C_PREPARE * g, "norminfd of the structured cone")
    km.within(k.get_W(i), *p["wsqrt"], km.C_PREPARE * g, "w^1/2 of the structured cone")
    for name in others:
        assert soc.same_bits(info[ids[name]], info0[ids0[name]]), name
    step = 0.5
    k.take_step(step, 1.0)
    alone.take_step(step, 1.0)
    Wn, Wm = km.ref_take(st, y, step)
    km.within(k.get_W(i), Wn, Wm, km.C_TAKE * g, "W after the step of the structured cone")
    for name in others:
        assert soc.same_bits(k.get_W(ids[name]), alone.get_W(ids0[name])), name


# ------------------------------------------------------------------------------------ refusals
def refusal_cases():
    """(name, keyword changes to a good call, the message): every refusal of cxk_add_quadratic_structured."""
    n = 4
    ptr = np.array([0, 1, 2, 3, 4], dtype=np.int32)
    idx = np.arange(n, dtype=np.int32)
    val = np.full(n, 2.0)
    F = np.full((n, 2), 0.5)
    good = dict(S=(ptr, idx, val), F=F, sigma=np.ones(2))
    nan = np.array([2.0, np.nan, 2.0, 2.0])
    return n, good, [
        ("rowptr-start", dict(S=(ptr + 1, np.arange(5, dtype=np.int32) % n, np.full(5, 2.0))), r"q_rowptr\[0\] is not 0"),
        ("rowptr-decreases", dict(S=(np.array([0, 2, 1, 3, 4], dtype=np.int32), idx, val)), r"q_rowptr decreases"),
        ("column-high", dict(S=(ptr, np.array([0, 1, 2, n], dtype=np.int32), val)), r"a column of the sparse part is outside \[0, n\)"),
        ("column-negative", dict(S=(ptr, np.array([0, -1, 2, 3], dtype=np.int32), val)), r"a column of the sparse part is outside \[0, n\)"),
        ("value-nan", dict(S=(ptr, idx, nan)), r"q_val holds a value that is not finite"),
        ("value-inf", dict(S=(ptr, idx, np.where(np.isnan(nan), np.inf, nan))), r"q_val holds a value that is not finite"),
        ("F-nan", dict(F=np.where(np.arange(8).reshape(n, 2) == 3, np.nan, 0.5)), r"F holds a value that is not finite"),
        ("sigma-inf", dict(sigma=np.array([1.0, -np.inf])), r"sigma holds a value that is not finite"),
        ("both-absent", dict(S=None, F=None, sigma=None), r"neither a sparse part nor factors.*Q = NULL.*cxk_add_quadratic"),
    ]


def check_refusals(device):
    n, good, cases = refusal_cases()
    A = np.full((n + 1, 2), 0.01)
    c = np.r_[1.0, np.zeros(n)]
    k = KktContext(2, device=device)
    for name, change, message in cases:
        kw = dict(good, **change)
        with pytest.raises(KktError, match=r"cxk_add_quadratic_structured: " + message):
            k.add_quadratic_structured(kw["S"], kw["F"], kw["sigma"], A, c)
    # rank < 0 cannot be said through an (n, r) array: the C entry point itself
    from conex_amd.kkt import _dp, _ip
    ptr, idx, val = good["S"]
    a = np.ascontiguousarray(A.T).ravel()
    assert k.L.cxk_add_quadratic_structured(k.h, n, 2, _ip(ptr), _ip(idx), _dp(val), -1, None, None, _dp(a), _dp(c), None) == -1
    assert k.L.cxk_last_error(k.h).decode() == "cxk_add_quadratic_structured: rank is negative"
    # the context stays usable
    assert k.add_quadratic_structured(good["S"], good["F"], good["sigma"], A, c) == 0
    k.initialize()
    return k


def test_every_refusal_raises_with_its_message_and_the_context_stays_usable():
    k = check_refusals(0)
    assert k.count_structured_quadratic() == 1
    k.assemble()
    assert np.all(np.isfinite(k.constraint_schur(0)[0]))
