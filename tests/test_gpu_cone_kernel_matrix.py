"""The kernels of the cones that are not matrices -- linear, second-order, quadratic, octonion, constant
block, line search (kernels_linear / _soc / _quad / _oct / _stage .hip.h) -- at their launch edges, against the
extended-precision reference of cone_reference.py.

Each row of ROWS is a handful of equal cones in a chain of cliques.  It runs at three scaling points
(the suite's usual ones, eigenvalue ratio 1e6 and 1e10, every W scaled to lambda_max = 1) through the
stages in order: assemble -> constraint_schur of every constraint -> eigenvalue query -> PrepareStep
(step_info per constraint, get_W) -> TakeStep at min(1, 2 / norminfd^2) (get_W), and for linear cones
the affine update.  Results are compared entry by entry, |gpu - ref| <= c u g * (magnitude sum), with
the constants of test_gpu_lmi_kernel_matrix.py and the reference's conditioning factor g
(cone_reference.py says what both are).  run_rows() is the whole comparison and takes the context
class: test_cone_reference.py runs it on the float64 oracle, which shows that correct float64 code
meets these bounds.  The last test recomputes every second-order row's launch shape with the launch
site's arithmetic, so that a row cannot change its path unnoticed.
"""
import numpy as np
import pytest

import cone_reference as ref
import oracle_lib as ol
from conex_amd import KktContext
from conex_amd.kkt import KktError
from conex_amd import synthetic as syn
from lmi_reference import lu_solve

pytestmark = pytest.mark.gpu

U = ref.U64
C_SCHUR = 64      # G, AW, AQc, the two scalars
C_PREPARE = 64    # normsqrd, norminfd, the w^{1/2} PrepareStep leaves in W, the query's four outputs
C_AFFINE = 32     # the linear cone's affine update
C_TAKE = 256      # W after the step, from the device's own d
POINTS = ("well", 1e6, 1e10)
C_WEIGHT = 1.0
K_LDS_LIMIT = 160 * 1024 - 512   # kLdsLimit (cone_route.h); 8 * 5104 * 4 = 8 * 88 * 58 * 4 = 163 328

# (id, kind, K, n, m, extra): soc / quad have dimension len = n + 1, lin has n rows, oct has order n;
# extra: quad "Q" / None, static "eq" (the equality path: a non-zero constant AQc) / None
ROWS = [
    ("soc-min", "soc", 1, 1, 1, None),                # smallest cone
    ("soc-base", "soc", 5, 10, 10, None),             # staged; the last workgroup has one live wavefront
    ("soc-len65", "soc", 4, 64, 8, None),             # lane loops wrap once
    ("soc-len129", "soc", 3, 128, 6, None),           # lane loops wrap twice
    ("soc-m65", "soc", 2, 4, 65, None),               # m loops and the m * m loop wrap
    ("soc-staged-edge", "soc", 5, 87, 27, None),      # len (2 m + 4) = 5104: the last staged shape
    ("soc-unstaged-w4", "soc", 5, 87, 28, None),      # the first unstaged shape, w = 4
    ("soc-unstaged-w3", "soc", 4, 199, 30, None),     # w = 3, K no multiple of w
    ("soc-unstaged-w2", "soc", 3, 299, 30, None),     # w = 2
    ("soc-unstaged-w1", "soc", 2, 599, 32, None),     # w = 1
    ("soc-admit-edge", "soc", 1, 318, 62, None),      # len (m + 2) = 20416: the last admitted shape
    ("soc-take-64k", "soc", 2, 2048, 2, None),        # soc_take_step above 64 KB of LDS
    ("soc-prepare-64k", "soc", 1, 2730, 2, None),     # soc_prepare above 64 KB as well
    ("soc-take-edge", "soc", 1, 5103, 1, None),       # 4 len = 20416 doubles: the last shape soc_take_step holds
    ("lin-min", "lin", 1, 1, 1, None),                # smallest; lanes without rows in the query
    ("lin-base", "lin", 5, 20, 10, None),
    ("lin-r256", "lin", 2, 256, 3, None),             # exactly one pass of 256 threads
    ("lin-r257", "lin", 2, 257, 3, None),             # one row in the second pass
    ("lin-r1000", "lin", 2, 1000, 3, None),           # four passes
    ("lin-m17", "lin", 2, 30, 17, None),              # m * m = 289 > 256 threads
    ("lin-m65", "lin", 1, 70, 65, None),
    ("quad-min", "quad", 1, 1, 1, "Q"),
    ("quad-q", "quad", 3, 5, 4, "Q"),
    ("quad-noq", "quad", 3, 5, 4, None),
    ("quad-n64-m65", "quad", 2, 64, 65, "Q"),
    ("quad-64k", "quad", 2, 2048, 2, None),           # the step kernels above 64 KB
    ("quad-prepare-edge", "quad", 1, 5102, 4, None),  # m + 4 len = 20416 doubles: the last shape quad_prepare holds
    ("oct-1", "oct", 1, 1, 1, None),
    ("oct-2", "oct", 2, 2, 5, None),
    ("oct-3", "oct", 2, 3, 9, None),
    ("oct-3-m27", "oct", 1, 3, 27, None),             # the full dimension of the algebra; m * m > 64 lanes
    ("static-m1", "static", 1, 0, 1, None),
    ("static-m9", "static", 2, 0, 9, None),           # m * m > 64 threads
    ("static-eq-m2", "static", 1, 0, 2, "eq"),        # one equality row over one variable: AQc = [0; b]
    ("static-eq-m9", "static", 1, 0, 9, "eq"),        # four rows over five variables
    ("mixed", "mixed", 1, 0, 6, None),                # one cone of each kind in one context
]
ROW_IDS = [r[0] for r in ROWS]
# Rows whose y is eight times the usual one: norminfd passes sqrt(2), the step length min(1, 2 / norminfd^2) falls
# below 1 and TakeStep scales d (and, for the second-order cone, writes it back) -- asserted where it is computed.
# (Other rows may take a short step as well; the octonion cone's heuristic norminfd stays small, so it takes its
# short step in the mixed row, where the other cones set the length.)
SHORT_STEP_ROWS = ("soc-len65", "soc-unstaged-w3", "quad-q", "quad-64k", "lin-r257", "mixed")


def soc_launch_shape(n, m):
    """LaunchSchur's choice for a second-order cone, restated: 'staged' or the unstaged workgroup width."""
    staged, plain = 8 * (n + 1) * (2 * m + 4), 8 * (n + 1) * (m + 2)
    if 4 * staged <= K_LDS_LIMIT:
        return "staged"
    return "unstaged-w%d" % max(1, min(4, K_LDS_LIMIT // plain))


# ------------------------------------------------------------------------------------ problems
def make_cone(kind, n, m, extra, point, rng):
    """One cone: its data, its scaling point W and the reference's functions of it."""
    if kind == "lin":
        return dict(kind=kind, m=m, A=rng.uniform(-1, 1, (n, m)), c=np.abs(rng.uniform(-1, 1, n)) + 0.1,
                    W=ref.lin_scaling_point(rng, n, point))
    if kind in ("soc", "quad"):
        c = 0.2 * rng.uniform(-1, 1, n + 1)
        c[0] = 1.0
        Q = None
        if extra == "Q":
            R = rng.uniform(-1, 1, (n, n))
            Q = R @ R.T / n + np.eye(n) if point == "well" else ref.conditioned_Q(rng, n, 1e6)
        return dict(kind=kind, m=m, A=rng.uniform(-1, 1, (n + 1, m)), c=c, Q=Q, W=ref.spin_scaling_point(rng, n, point, Q))
    if kind == "oct":
        C = np.zeros((8, n, n))
        C[0] = np.eye(n)
        return dict(kind=kind, m=m, A=np.array([ref.oct_random_hermitian(rng, n) for _ in range(m)]), C=C,
                    W=ref.oct_scaling_point(rng, n, point))
    if extra == "eq":
        rows = 1 if m == 2 else 4
        return dict(kind="eq", m=m, A=rng.uniform(-1, 1, (rows, m - rows)), b=rng.uniform(-1, 1, rows))
    R = rng.uniform(-1, 1, (m, m))
    return dict(kind="static", m=m, G=R @ R.T + m * np.eye(m))


def make_problem(row, point, seed):
    """(cones, cliques, num_vars): K equal cones in a chain of cliques; a constant block shares its variables
    with a small linear cone; the mixed row is one cone of each kind over the same six variables."""
    _, kind, K, n, m, extra = row
    rng = np.random.default_rng(seed)
    if kind == "mixed":
        shapes = [("lin", 7, m, None), ("soc", 6, m, None), ("quad", 5, m, "Q"), ("oct", 2, m, None), ("static", 0, m, None)]
        return [make_cone(k, nn, mm, ex, point, rng) for k, nn, mm, ex in shapes], [list(range(m))] * 5, m
    if kind == "static":
        user = m - (0 if extra != "eq" else (1 if m == 2 else 4))
        cliques, num_vars = syn.chain_cliques(K, user, 1 if user > 1 else 0)
        cones = [make_cone(kind, n, m, extra, point, rng) for _ in range(K)]
        return cones + [make_cone("lin", 3, user, None, point, rng)], cliques + [cliques[0]], num_vars
    cliques, num_vars = syn.chain_cliques(K, m, 1 if m > 1 else 0)
    return [make_cone(kind, n, m, extra, point, rng) for _ in range(K)], cliques, num_vars


def build(cls, cones, cliques, num_vars, **kw):
    p = cls(num_vars, **kw)
    for i, (cn, cl) in enumerate(zip(cones, cliques)):
        k = cn["kind"]
        r = (p.add_linear(cn["A"], cn["c"], cl) if k == "lin" else p.add_soc(cn["A"], cn["c"], cl) if k == "soc" else
             p.add_quadratic(cn["Q"], cn["A"], cn["c"], cl) if k == "quad" else p.add_hermitian(cn["A"], cn["C"], cl) if k == "oct" else
             p.add_equality(cn["A"], cn["b"], cl) if k == "eq" else p.add_static(cn["G"], cl))
        assert r == i, (k, r)
    p.initialize()
    return p


def set_points(p, cones):
    for i, cn in enumerate(cones):
        if "W" in cn:
            p.set_W(i, cn["W"])


def is_cone(cn):
    return cn["kind"] not in ("static", "eq")


# ------------------------------------------------------------------------------------ reference
def ref_schur(cn):
    k = cn["kind"]
    if k == "lin":
        return ref.lin_schur(cn["A"], cn["c"], cn["W"])
    if k == "soc":
        return ref.soc_schur(cn["A"], cn["c"], cn["W"])
    if k == "quad":
        return ref.quad_schur(cn["A"], cn["c"], cn["W"], cn["Q"])
    return ref.oct_schur(cn["A"], cn["C"], cn["W"])


def ref_query(cn, z):
    k = cn["kind"]
    if k == "lin":
        return ref.lin_query(cn["A"], cn["c"], cn["W"], z, C_WEIGHT)
    if k == "oct":
        return ref.oct_query(cn["A"], cn["C"], cn["W"], z, C_WEIGHT)
    return ref.spin_query(cn["A"], cn["c"], cn["W"], z, C_WEIGHT, cn.get("Q"))


def ref_prepare(cn, z):
    k = cn["kind"]
    if k == "lin":
        return ref.lin_prepare(cn["A"], cn["c"], cn["W"], z, C_WEIGHT, 1.0)
    if k == "oct":
        return ref.oct_prepare(cn["A"], cn["C"], cn["W"], z, C_WEIGHT)
    return ref.spin_prepare(cn["A"], cn["c"], cn["W"], z, C_WEIGHT, cn.get("Q"), quad=k == "quad")


def ref_take(cn, z, step):
    k = cn["kind"]
    if k == "lin":
        return ref.lin_take(cn["A"], cn["c"], cn["W"], z, C_WEIGHT, 1.0, step)
    if k == "oct":
        return ref.oct_take(cn["A"], cn["C"], cn["W"], z, C_WEIGHT, step)
    return ref.spin_take(cn["A"], cn["c"], cn["W"], z, C_WEIGHT, step, cn.get("Q"))


def within(got, val, mag, c, what, report=None):
    got = np.asarray(got, dtype=np.float64)
    val, mag = np.broadcast_to(val, got.shape), np.broadcast_to(mag, got.shape)
    err = np.abs(got.astype(ref.LD) - val)
    bound = c * U * mag
    worst = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny))) if got.size else 0.0
    if report is not None:
        report.append((what, worst))
    assert np.all(err <= bound), f"{what}: error {worst:.3g} x the bound c u g |.| (c g = {c:.3g})"


def slack_scale(cn, z):
    if cn["kind"] == "oct":
        return float(np.max(np.tensordot(np.abs(z), np.abs(cn["A"]), axes=1)))
    return float(np.max(np.abs(cn["A"]) @ np.abs(z)))


def make_y(cones, cliques, num_vars, seed, short_step=False):
    """The fixed y of a row (an equality block's multipliers follow the variables: no kernel reads them): the
    slack's A y part at most 0.5 in every cone, or 4 where the row is to take a step below 1."""
    N = num_vars + sum(cn["A"].shape[0] for cn in cones if cn["kind"] == "eq")
    y = np.random.default_rng(seed).uniform(-1, 1, N)
    y[:num_vars] *= (4.0 if short_step else 0.5) / max(slack_scale(cn, y[cl]) for cn, cl in zip(cones, cliques) if is_cone(cn))
    return y


def step_length(prepared):
    """min(1, 2 / norminfd^2) of the reference's reduced norminfd, as check_newton_step takes it."""
    ninf = float(max(p["norminfd"][0] for p in prepared.values()))
    return min(1.0, 2.0 / ninf ** 2)


def run_rows(cls, cones, cliques, num_vars, seed, report=None, short_step=False, **kw):
    """Every stage of every cone on a context of class `cls` (KktContext, or the float64 oracle) against the reference."""
    k = build(cls, cones, cliques, num_vars, **kw)
    set_points(k, cones)
    K = len(cones)
    y = make_y(cones, cliques, num_vars, seed, short_step)
    assert len(y) == k.N
    z = [y[cl] for cl in cliques]

    # Schur complement
    k.assemble()
    for i, cn in enumerate(cones):
        G, AW, AQc, sc = k.constraint_schur(i)
        if not is_cone(cn):  # the constant block: a copy, bit for bit
            if cn["kind"] == "eq":
                rows, user = cn["A"].shape
                Gc = np.zeros((cn["m"], cn["m"]))
                Gc[user:, :user] = cn["A"]
                Gc[:user, user:] = cn["A"].T
                r = ref.static_schur(Gc, np.r_[np.zeros(user), cn["b"]])
            else:
                r = ref.static_schur(cn["G"])
            assert np.array_equal(G, r["G"]) and np.array_equal(AW, r["AW"]) and np.array_equal(AQc, r["AQc"])
            assert np.array_equal(sc, r["sc"])
            continue
        r = ref_schur(cn)
        low = np.tril(np.ones_like(G, dtype=bool))
        within(G[low], r["G"][0][low], r["G"][1][low], C_SCHUR * r["g"], f"G of constraint {i}", report)
        within(AW, *r["AW"], C_SCHUR, f"AW of constraint {i}", report)
        within(AQc, *r["AQc"], C_SCHUR * r["g"], f"AQc of constraint {i}", report)
        within(sc, *r["sc"], C_SCHUR * r["g"], f"scalars of constraint {i}", report)

    live = [i for i, cn in enumerate(cones) if is_cone(cn)]

    def reduced(vals, name, how):
        """A reduction of per-constraint (value, magnitude) pairs, in ids order, and the bound that goes with it."""
        v = [vals[i][name][0] for i in live]
        b = [vals[i][name][1] * vals[i]["g"] for i in live]
        if how == "sum":
            return sum(v), sum(b)
        return (max(v) if how == "max" else min(v)), max(b)

    # the eigenvalue query: min lmin, max lmax, sum frob, sum trace over the constraints
    q = {i: ref_query(cones[i], z[i]) for i in live}
    ek = k.weighted_slack_eigenvalues(y, C_WEIGHT)
    for j, (name, how) in enumerate((("lmin", "min"), ("lmax", "max"), ("frob", "sum"), ("trace", "sum"))):
        within(ek[j], *reduced(q, name, how), C_PREPARE, f"query {name}", report)

    # PrepareStep
    p = {i: ref_prepare(cones[i], z[i]) for i in live}
    ik = k.prepare_step(y, C_WEIGHT, 1.0)
    within(ik[0], *reduced(p, "normsqrd", "sum"), C_PREPARE, "normsqrd", report)
    within(ik[1], *reduced(p, "norminfd", "max"), C_PREPARE, "norminfd", report)
    if hasattr(k, "step_info"):
        info = k.step_info()
        for i in range(K):
            if i not in p:
                assert info[i, 0] == 0 and info[i, 1] == 0  # a constant block keeps StepInfo {0, 0}
                continue
            within(info[i, 0], p[i]["normsqrd"][0], p[i]["normsqrd"][1], C_PREPARE * p[i]["g"], f"normsqrd of constraint {i}", report)
            within(info[i, 1], p[i]["norminfd"][0], p[i]["norminfd"][1], C_PREPARE * p[i]["g"], f"norminfd of constraint {i}", report)
    for i in live:
        if "wsqrt" in p[i]:
            within(k.get_W(i), *p[i]["wsqrt"], C_PREPARE * p[i]["g"], f"w^1/2 of constraint {i}", report)

    # TakeStep with the reference's step length
    step = step_length(p)
    assert step < 1.0 or not short_step, step
    k.take_step(step, 1.0)
    for i in live:
        Wn, Wm = ref_take(cones[i], z[i], step)
        within(k.get_W(i).reshape(np.shape(Wn)), Wn, Wm, C_TAKE * p[i]["g"], f"W after the step {step:.3g} of constraint {i}", report)

    # the affine update (linear cones)
    lin = [i for i in live if cones[i]["kind"] == "lin"]
    if lin:
        set_points(k, cones)
        k.prepare_step(y, C_WEIGHT, 0.3, affine=1)
        for i in lin:
            Wa, Wm = ref.lin_affine(cones[i]["A"], cones[i]["c"], cones[i]["W"], z[i])
            within(k.get_W(i), Wa, Wm, C_AFFINE, f"affine W of constraint {i}", report)
    return report


def row_seed(row):
    _, _, K, n, m, _ = row
    return 2000 + 31 * n + 7 * m + K


@pytest.mark.parametrize("point", POINTS, ids=lambda p: p if isinstance(p, str) else f"cond{p:.0e}")
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_cone_kernel_matrix(row, point):
    cones, cliques, num_vars = make_problem(row, point, row_seed(row))
    run_rows(KktContext, cones, cliques, num_vars, row_seed(row) + 1, short_step=row[0] in SHORT_STEP_ROWS, device=0)


# ------------------------------------------------------------------------------------ refusals
def soc_data(n, m):
    c = np.zeros(n + 1)
    c[0] = 1.0
    return np.full((n + 1, m), 0.01), c


@pytest.mark.parametrize("kind,n,m", [("soc", 319, 62),    # len (m + 2) = 20480: one past the admission edge
                                      ("soc", 5104, 1),    # 4 len = 20420 doubles: one past soc_take_step's
                                      ("quad", 5103, 4),   # m + 4 len = 20420 doubles: one past quad_prepare's
                                      ("quad", 6804, 1)])  # (what the second-order cone's image rule alone would admit)
def test_cones_beyond_lds_are_refused_at_initialize(kind, n, m):
    A, c = soc_data(n, m)
    k = KktContext(m, device=0)
    assert (k.add_soc(A, c) if kind == "soc" else k.add_quadratic(None, A, c)) == 0
    with pytest.raises(KktError, match=r"LDS"):
        k.initialize()


# ------------------------------------------------------------------------------------ line search
LS_CASES = [(20, 0), (20, 19), (257, 0), (257, 255), (257, 256), (1000, 255), (1000, 256), (1000, 999)]


def line_search_problem(r, bind, seed=5):
    """A linear cone of r rows over three variables and a quadratic-cost block; row `bind` of (A, c) is scaled up so
    that it ends the admissible interval.  The cost block is heavy enough (it grows with r) that the two solves do not
    bend towards that one row, which would shrink its delta again."""
    rng = np.random.default_rng(seed + r + bind)
    m = 3
    A = rng.uniform(-1, 1, (r, m))
    c = np.abs(rng.uniform(-1, 1, r)) + 0.1
    A[bind] *= 6.0
    c[bind] = 6.0
    R = rng.uniform(-1, 1, (m, m))
    G = (r + 40.0) * (R @ R.T / m + np.eye(m))
    cones = [dict(kind="lin", m=m, A=A, c=c, W=rng.uniform(0.5, 1.0, r)), dict(kind="static", m=m, G=G)]
    return cones, [list(range(m))] * 2, m, rng.uniform(-1, 1, m)


def line_search_reference(cones, cliques, num_vars, b, b_scaling, c_scaling):
    """(lower ends, upper ends, delta, d0) per row, from the oracle's assembled system solved in longdouble."""
    o = build(ol.Program, cones, cliques, num_vars)
    set_points(o, cones)
    o.assemble()
    Kmat = ref.ld(o.kkt_matrix())
    AW, AQc, _ = o.residuals()
    AW, AQc = ref.ld(AW), ref.ld(AQc)
    rhs = np.stack([-2 * AW, AQc * ref.LD(c_scaling) + ref.ld(b) * ref.LD(b_scaling) - 2 * AW], axis=1)
    Y = lu_solve(Kmat, rhs)
    cn = cones[0]
    d0 = (ref.ld(cn["A"]) @ Y[:, 0]) * ref.ld(cn["W"]) + 1
    return Y, d0


def line_search_expected(r, bind, b_scaling=0.9, c_scaling=0.8):
    """The problem, dinf (half again the largest |d0|: t = 0 is admissible) and the reference's interval ends,
    with the precondition under which a wrong row is distinguishable from rounding asserted."""
    cones, cliques, num_vars, b = line_search_problem(r, bind)
    Y, d0 = line_search_reference(cones, cliques, num_vars, b, b_scaling, c_scaling)
    dinf = float(1.5 * np.max(np.abs(d0)))
    cn = cones[0]
    lbs, ubs, delta = ref.lin_line_search(cn["A"], cn["c"], cn["W"], Y[:, 0], Y[:, 1], c_scaling, dinf)
    order = np.argsort(ubs)
    assert order[0] == bind, (order[:3], bind)
    assert abs(delta[bind]) >= 0.1 * np.max(np.abs(delta))
    if r > 1:
        assert ubs[order[1]] - ubs[bind] >= 1e-3 * abs(ubs[bind])
    return cones, cliques, num_vars, b, dinf, ref.line_search_result([lbs], [ubs]), (b_scaling, c_scaling)


@pytest.mark.parametrize("r,bind", LS_CASES)
def test_line_search_takes_the_binding_row(r, bind):
    cones, cliques, num_vars, b, dinf, want, (bs, cs) = line_search_expected(r, bind)
    assert want > 0
    k = build(KktContext, cones, cliques, num_vars, device=0)
    set_points(k, cones)
    k.set_cost(b)
    k.assemble()
    assert k.factor() == 1
    got = k.line_search(dinf, bs, cs)
    assert abs(got - float(want)) <= 1e-9 * abs(float(want)), (got, float(want))
    # an interval no step fits
    assert k.line_search(1e-6, bs, cs) == -1.0


def test_line_search_refuses_a_second_order_cone():
    cones, cliques, num_vars, b, dinf, _, (bs, cs) = line_search_expected(20, 0)
    rng = np.random.default_rng(3)
    cones = cones + [make_cone("soc", 4, 3, None, "well", rng)]
    k = build(KktContext, cones, cliques + [cliques[0]], num_vars, device=0)
    set_points(k, cones)
    k.set_cost(b)
    k.assemble()
    assert k.factor() == 1
    assert k.line_search(dinf, bs, cs) == -1.0


# ------------------------------------------------------------------------------------ completeness
def test_the_rows_cover_every_kind_and_every_second_order_launch_shape():
    kinds = {r[1] for r in ROWS}
    assert kinds >= {"soc", "lin", "quad", "oct", "static", "mixed"}
    shapes = {r[0]: soc_launch_shape(r[3], r[4]) for r in ROWS if r[1] == "soc"}
    assert set(shapes.values()) == {"staged", "unstaged-w4", "unstaged-w3", "unstaged-w2", "unstaged-w1"}
    for rid, shape in shapes.items():  # a row named after a shape runs it
        if "unstaged" in rid:
            assert shape == rid[len("soc-"):], (rid, shape)
    assert shapes["soc-staged-edge"] == "staged" and 8 * 88 * (2 * 27 + 4) * 4 == K_LDS_LIMIT
    assert shapes["soc-base"] == shapes["soc-len65"] == shapes["soc-len129"] == shapes["soc-m65"] == "staged"
    assert 8 * 319 * (62 + 2) == K_LDS_LIMIT and 8 * 4 * 5104 == K_LDS_LIMIT and 8 * (4 + 4 * 5103) == K_LDS_LIMIT
    # every K that leaves the last workgroup partly empty at its width
    assert any(r[1] == "soc" and soc_launch_shape(r[3], r[4]) == "staged" and r[2] % 4 for r in ROWS)
    assert any(r[0] == "soc-unstaged-w3" and r[2] % 3 for r in ROWS)
