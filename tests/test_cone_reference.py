"""The extended-precision cone reference (cone_reference.py) against the CPU oracle.

First at well-conditioned points, to 1e-13 norm-relative, for every kind and every stage: if the
reference is wrong, this says so before any kernel comparison is read.  Then the float64 oracle is put
through the whole comparison of test_gpu_cone_kernel_matrix.py -- every row, every scaling point, the
same entrywise bounds: correct float64 code meets them, which is what justifies their constants.  The
line-search cases' precondition (the binding row is well separated) is checked here too.
"""
import functools

import numpy as np
import pytest

import cone_reference as ref
import oracle_lib as ol
import test_gpu_cone_kernel_matrix as km
from conex_amd import synthetic as syn

TOL = 1e-13


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    n = np.linalg.norm(b)
    return np.linalg.norm(a - b) / n if n > 0 else np.linalg.norm(a - b)


PINS = [("lin", 20, 6, None), ("lin", 300, 3, None), ("soc", 10, 7, None), ("soc", 70, 3, None), ("quad", 5, 4, "Q"),
        ("quad", 6, 3, None), ("oct", 3, 5, None), ("oct", 2, 3, None)]


def one_cone(kind, n, m, extra, seed):
    rng = np.random.default_rng(seed)
    cn = km.make_cone(kind, n, m, extra, "well", rng)
    o = km.build(ol.Program, [cn], [list(range(m))], m)
    km.set_points(o, [cn])
    return cn, o, rng.uniform(-0.1, 0.1, m)


@pytest.mark.parametrize("kind,n,m,extra", PINS)
def test_schur_matches_the_oracle(kind, n, m, extra):
    cn, o, _ = one_cone(kind, n, m, extra, 11 + n + m)
    r = km.ref_schur(cn)
    o.assemble()
    Go, AWo, AQo, sco = o.constraint_schur(0)
    assert rel(np.tril(np.asarray(r["G"][0], dtype=np.float64)), np.tril(Go)) <= TOL
    assert rel(r["AW"][0], AWo) <= TOL and rel(r["AQc"][0], AQo) <= TOL and rel(r["sc"][0], sco) <= TOL
    for name in ("G", "AW", "AQc", "sc"):  # a magnitude sum bounds its value
        v, mag = r[name]
        assert np.all(np.abs(v) <= mag * (1 + 1e-15))


@pytest.mark.parametrize("kind,n,m,extra", PINS)
def test_query_prepare_take_and_affine_match_the_oracle(kind, n, m, extra):
    cn, o, y = one_cone(kind, n, m, extra, 23 + n + m)
    c = km.C_WEIGHT
    q, p = km.ref_query(cn, y), km.ref_prepare(cn, y)
    eo = o.weighted_slack_eigenvalues(y, c)
    for j, name in enumerate(("lmin", "lmax", "frob", "trace")):
        assert rel(q[name][0], eo[j]) <= TOL, name
    io = o.prepare_step(y, c, 1.0)
    assert rel(p["normsqrd"][0], io[0]) <= TOL and rel(p["norminfd"][0], io[1]) <= TOL
    if "wsqrt" in p:
        assert rel(p["wsqrt"][0], o.get_W(0)) <= TOL
    step = min(1.0, 2.0 / io[1] ** 2) * 0.9
    Wn, Wm = km.ref_take(cn, y, step)
    o.take_step(step, 1.0)
    assert rel(Wn, o.get_W(0)) <= TOL
    assert np.all(np.abs(Wn) <= Wm * (1 + 1e-15))
    if kind == "lin":
        o.set_W(0, cn["W"])
        o.prepare_step(y, c, 0.3, affine=1)
        assert rel(ref.lin_affine(cn["A"], cn["c"], cn["W"], y)[0], o.get_W(0)) <= TOL


def test_the_octonion_table_is_the_projects_own():
    assert np.array_equal(ref.OCT_SIGN, syn.HC_SIGN)
    rng = np.random.default_rng(1)
    X, Y = rng.uniform(-1, 1, (2, 8, 3, 3))
    assert np.allclose(np.asarray(ref.oct_mul(ref.ld(X), ref.ld(Y)), dtype=np.float64), syn.hc_multiply(X, Y), atol=1e-14)


@pytest.mark.parametrize("point", [1e6, 1e10])
def test_scaling_points_have_the_spectrum_asked_for(point):
    rng = np.random.default_rng(4)
    w = ref.lin_scaling_point(rng, 50, point)
    assert w.max() == 1.0 and 1.0 / point <= w.min() < 1e-2
    Q = ref.conditioned_Q(rng, 7, 1e6)
    assert abs(np.log10(np.linalg.cond(Q)) - 6) < 0.01
    for q in (None, Q):
        lo, hi = ref.spin_eigs(ref.spin_scaling_point(rng, 7, point, q), q)
        assert abs(float(hi) - 1) < 1e-9 and abs(float(lo) * point - 1) < 1e-4
        assert abs(ref.spin_g(ref.spin_scaling_point(rng, 7, point, q), q) / np.sqrt(point) - 1) < 1e-4


POINT_IDS = [p if isinstance(p, str) else f"cond{p:.0e}" for p in km.POINTS]
ROW_OF = {r[0]: r for r in km.ROWS}


@functools.lru_cache(maxsize=None)
def oracle_report(row_id, point):
    """[(quantity, error / bound)] of the float64 oracle in the GPU file's whole comparison (which asserts as it goes)."""
    row = ROW_OF[row_id]
    cones, cliques, num_vars = km.make_problem(row, point, km.row_seed(row))
    return km.run_rows(ol.Program, cones, cliques, num_vars, km.row_seed(row) + 1, [], short_step=row_id in km.SHORT_STEP_ROWS)


@pytest.mark.parametrize("point", km.POINTS, ids=POINT_IDS)
@pytest.mark.parametrize("row", km.ROWS, ids=km.ROW_IDS)
def test_the_float64_oracle_meets_the_gpu_bounds(row, point):
    assert oracle_report(row[0], point)


def test_the_bounds_are_not_slack():
    """Below the bound is not enough: over the rows of a kind the float64 oracle comes within 1e-3 .. 1 of the bound
    of every quantity.  A bound orders of magnitude too wide would leave it far below.  (The mixed row is left out:
    one context, whose reduced quantities sum over the kinds.)"""
    worst = {}
    for row in km.ROWS:
        for point in km.POINTS:
            for what, ratio in oracle_report(row[0], point):
                key = (row[1], what.split(" of constraint")[0].split(" after the step")[0])
                worst[key] = max(worst.get(key, 0.0), ratio)
    print({k: f"{v:.2g}" for k, v in sorted(worst.items())})
    low = {k: v for k, v in worst.items() if k[0] != "mixed" and not 1e-3 <= v <= 1.0}
    assert not low, low


@pytest.mark.parametrize("point", km.POINTS, ids=POINT_IDS)
@pytest.mark.parametrize("row", km.ROWS, ids=km.ROW_IDS)
def test_grossly_wrong_results_fail_the_bounds(row, point):
    """At every row and point the comparison refuses W left unchanged by TakeStep (as set, and as PrepareStep leaves
    it), W = 0, a normsqrd formed from d without the + e, a norminfd that is the other eigenvalue's, and a w^{1/2}
    that is W: no bound is so wide that it accepts anything."""
    cones, cliques, num_vars = km.make_problem(row, point, km.row_seed(row))
    short = row[0] in km.SHORT_STEP_ROWS
    y = km.make_y(cones, cliques, num_vars, km.row_seed(row) + 1, short)
    live = [i for i, cn in enumerate(cones) if km.is_cone(cn)]
    z = {i: y[cliques[i]] for i in live}
    p = {i: km.ref_prepare(cones[i], z[i]) for i in live}
    step = km.step_length(p)

    def refused(got, val, mag, c, what):
        with pytest.raises(AssertionError):
            km.within(got, val, mag, c, what)

    for i in live:
        cn, g = cones[i], p[i]["g"]
        W = np.asarray(cn["W"], dtype=np.float64)
        Wn, Wm = km.ref_take(cn, z[i], step)
        refused(W.reshape(np.shape(Wn)), Wn, Wm, km.C_TAKE * g, "W unchanged")
        refused(np.zeros(np.shape(Wn)), Wn, Wm, km.C_TAKE * g, "W = 0")
        q = km.ref_query(cn, z[i])  # (its frob is normsqrd's expression on d without the + e)
        if abs(q["frob"][0] - p[i]["normsqrd"][0]) > 1e-6 * p[i]["normsqrd"][0]:  # (order 1, s = -1/2: (s + 1)^2 = s^2)
            refused(float(q["frob"][0]), *p[i]["normsqrd"], km.C_PREPARE * g, "normsqrd without e")
        if "wsqrt" in p[i]:
            left = np.asarray(p[i]["wsqrt"][0], dtype=np.float64)
            refused(left, Wn, Wm, km.C_TAKE * g, "W as PrepareStep left it")
            refused(W, *p[i]["wsqrt"], km.C_PREPARE * g, "w^1/2 = W")
            d = p[i]["d"][0]
            kq = ref.qnorm(cn.get("Q"), d[1:], np.abs(d[1:]))[0]
            refused(float(min(abs(d[0] + kq), abs(d[0] - kq))), *p[i]["norminfd"], km.C_PREPARE * g, "the other eigenvalue")


@pytest.mark.parametrize("r,bind", km.LS_CASES)
def test_line_search_cases_are_well_separated(r, bind):
    """The precondition of the GPU line-search test (asserted inside line_search_expected), and that the
    bound its empty-interval case passes leaves no admissible step."""
    cones, cliques, num_vars, b, dinf, want, (bs, cs) = km.line_search_expected(r, bind)
    assert want > 0
    # a too-small bound leaves no step
    Y, _ = km.line_search_reference(cones, cliques, num_vars, b, bs, cs)
    cn = cones[0]
    lbs, ubs, _ = ref.lin_line_search(cn["A"], cn["c"], cn["W"], Y[:, 0], Y[:, 1], cs, 1e-6)
    assert ref.line_search_result([lbs], [ubs]) == -1


def test_launch_shapes_of_the_rows():
    km.test_the_rows_cover_every_kind_and_every_second_order_launch_shape()
