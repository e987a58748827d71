"""Quadratic cones whose (n + 1) x m matrix A is given by its nonzeros (cxk_add_quadratic_csr,
kernels_quad_sparse.hip.h), at the edges of the new kernels, against the extended-precision reference of
cone_reference.py.

The stages and the bounds are those of test_gpu_cone_kernel_matrix.py (run_rows / C_SCHUR, C_PREPARE, C_TAKE, imported
unchanged); the rows, their data and the context class are quad_sparse_cases.py's.  Each row runs at the three scaling
points on a SparseAQuad context, whose add_quadratic hands the nonzeros of the dense A to add_quadratic_csr: the
reference sees the dense A, the device never does.  test_quad_sparse_reference.py runs the same rows on the float64
oracle, which shows that correct float64 code meets the bounds at these shapes.

Beyond the dense form ((n + 1) m = 2^31 + 2048) the reference is quad_sparse_cases.quad_schur_op, cone_reference's
quad_schur restated for a CSR A; test_quad_sparse_reference.py pins it to quad_schur on every row.
"""
import numpy as np
import pytest

import cone_reference as ref
import quad_sparse_cases as qs
import quad_structured_cases as qc
import test_gpu_cone_kernel_matrix as km
import test_gpu_soc_streamed as soc
import test_quad_sparse_reference as host
from conex_amd import KktContext
from conex_amd import synthetic as syn

pytestmark = pytest.mark.gpu

POINT_IDS = [p if isinstance(p, str) else f"cond{p:.0e}" for p in km.POINTS]
STAGE_KEYS = ("schur", "query", "prepare", "info", "wsqrt", "W")


def counting(counted, base=qs.SparseAQuad):
    class Counting(base):
        def initialize(self):
            r = super().initialize()
            counted.append((self.count_sparse_quadratic(), self.count_streamed_quadratic()))
            return r

    return Counting


def test_rows_sit_on_their_edges():
    qs.test_rows_sit_on_their_edges()


@pytest.mark.parametrize("point", km.POINTS, ids=POINT_IDS)
@pytest.mark.parametrize("row", qs.ROWS, ids=qs.ROW_IDS)
def test_sparse_quadratic_kernel_matrix(row, point):
    cones, cliques, num_vars = qs.make_problem(row, point)
    counted = []
    km.run_rows(counting(counted), cones, cliques, num_vars, qs.row_seed(row) + 1, short_step=row[0] in qs.SHORT_STEP_ROWS, device=0)
    assert counted == [(row[1], row[1])]


# ------------------------------------------------------------------------------------ beyond the dense form
BIG_N, BIG_M, BIG_PER = 2 ** 20, 2048, 512


def big_problem():
    """n = 2^20, m = 2048: (n + 1) m = 2^31 + 2048.  Q a diagonal S plus rank 1; column j of A1 holds rows 512 j ..
    512 j + 511, A0 all ones; W well inside the cone."""
    rng = np.random.default_rng(2 ** 20)
    parts = dict(S=(np.arange(BIG_N + 1, dtype=np.int32), np.arange(BIG_N, dtype=np.int32), rng.uniform(1.0, 2.0, BIG_N)),
                 F=qc.make_f(BIG_N, 1, rng), sigma=rng.uniform(0.5, 1.5, 1))
    c = 0.2 * rng.uniform(-1, 1, BIG_N + 1)
    c[0] = 1.0
    indptr = np.r_[0, BIG_M + np.arange(BIG_N + 1)].astype(np.int32)  # row 0 full, one entry in every row of A1
    indices = np.r_[np.arange(BIG_M), np.arange(BIG_N) // BIG_PER].astype(np.int32)
    data = np.r_[np.ones(BIG_M), rng.uniform(-1, 1, BIG_N)]
    w1 = rng.uniform(-0.3, 0.3, BIG_N)
    k = float(np.sqrt(w1 @ qc.apply_q(parts, w1)))
    W = np.r_[k + rng.uniform(0.5, 1.5), w1]
    return parts, (indptr, indices, data), c, W / (W[0] + k)


def in_cone(parts, W):
    W = ref.ld(W)
    return bool(np.all(np.isfinite(W)) and W[0] > 0 and W[0] * W[0] > W[1:] @ qc.apply_q(parts, W[1:]))


def test_a_shape_beyond_the_dense_form():
    assert (BIG_N + 1) * BIG_M == 2 ** 31 + 2048 and BIG_N == BIG_M * BIG_PER
    parts, A, c, W = big_problem()
    k = KktContext(BIG_M, device=0)
    assert k.add_quadratic_csr(parts, A, c) == 0
    k.initialize()
    assert k.count_sparse_quadratic() == 1 and k.count_streamed_quadratic() == 1 and k.count_structured_quadratic() == 1
    k.set_W(0, W)
    k.assemble()
    G, AW, AQc, sc = k.constraint_schur(0)
    r = qs.quad_schur_op(A, BIG_M, c, W, parts=parts)
    low = np.tril(np.ones_like(G, dtype=bool))
    km.within(G[low], r["G"][0][low], r["G"][1][low], km.C_SCHUR, "G")
    km.within(AW, *r["AW"], km.C_SCHUR, "AW")
    km.within(AQc, *r["AQc"], km.C_SCHUR, "AQc")
    km.within(sc, *r["sc"], km.C_SCHUR, "scalars")
    y = np.random.default_rng(1).uniform(-1, 1, BIG_M)
    indptr, indices, data = A
    rows_scale = max(float(np.sum(np.abs(y))), float(np.max(np.abs(data[BIG_M:]) * np.abs(y)[indices[BIG_M:]])))  # max |A| |y|
    y *= 0.5 / rows_scale
    info = k.prepare_step(y, km.C_WEIGHT, 1.0)
    assert np.all(np.isfinite(info)) and info[1] > 0
    k.take_step(min(1.0, 2.0 / info[1] ** 2), 1.0)
    assert in_cone(parts, k.get_W(0))


# ------------------------------------------------------------------------------------ bits
def run_stages(cls, cones, cliques, num_vars, seed, take="separate"):
    return soc.run_stages(cls, cones, cliques, num_vars, seed, take)


@pytest.mark.parametrize("row_id", ["long-column", "panel"])
def test_two_runs_give_the_same_bits(row_id):
    row = qs.ROWS[qs.ROW_IDS.index(row_id)]
    cones, cliques, num_vars = qs.make_problem(row, 1e6)
    a = run_stages(qs.SparseAQuad, cones, cliques, num_vars, 5)
    b = run_stages(qs.SparseAQuad, cones, cliques, num_vars, 5)
    for key in STAGE_KEYS:
        assert soc.same_bits(a[key], b[key]), key


@pytest.mark.parametrize("row_id", ["group-of-3", "full-dense"])
def test_descending_columns_give_the_bits_of_ascending_input(row_id):
    row = qs.ROWS[qs.ROW_IDS.index(row_id)]
    cones, cliques, num_vars = qs.make_problem(row, 1e6)
    csr = qs.csr_of(cones[-1]["A"])
    assert not np.array_equal(qs.descending(csr)[1], csr[1])
    a = run_stages(qs.SparseAQuad, cones, cliques, num_vars, 6)
    b = run_stages(qs.DescendingSparseAQuad, cones, cliques, num_vars, 6)
    for key in STAGE_KEYS:
        assert soc.same_bits(a[key], b[key]), key


# ------------------------------------------------------------------------------------ the switch
@pytest.mark.parametrize("row_id", ["full-none", "full-dense", "full-parts"])
def test_streamed_mode_zero_does_not_refuse_the_cone(row_id):
    row = qs.ROWS[qs.ROW_IDS.index(row_id)]
    cones, cliques, num_vars = qs.make_problem(row, "well")
    cn = cones[0]
    k = qs.SparseAQuad(num_vars, device=0)
    k.set_streamed_quadratic(0)
    assert k.add_quadratic(cn["Q"], cn["A"], cn["c"], cliques[0]) == 0
    k.initialize()
    assert k.count_sparse_quadratic() == 1 and k.count_streamed_quadratic() == 1
    k.set_W(0, cn["W"])
    k.assemble()
    G, AW, AQc, sc = k.constraint_schur(0)
    r = km.ref_schur(cn)
    km.within(AW, *r["AW"], km.C_SCHUR, "AW")
    km.within(AQc, *r["AQc"], km.C_SCHUR * r["g"], "AQc")


# ------------------------------------------------------------------------------------ a mixed context
MIXED_MIN_WORK = 10000  # between the two dense-A quadratic cones below, as test_gpu_quad_streamed.MIXED_MIN_WORK


class MixedContext(qs.SparseAQuad):
    """Sparse-A for the cones marked so (an attribute of the A handed over), dense for the others."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.set_streamed_quadratic(-1)
        self.set_sparse_soc(-1)

    def add_quadratic(self, Q, A, c, vars_=None):
        if getattr(A, "by_nonzeros", False):
            return super().add_quadratic(Q, np.asarray(A), c, vars_)
        return KktContext.add_quadratic(self, Q, A, c, vars_)


class ByNonzeros(np.ndarray):
    by_nonzeros = True


def mixed_problem(point, seed):
    """One sparse-A cone (300, 62: tridiagonal plus rank 2, three entries per row), one dense-A streamed cone (128, 62),
    one LDS-route quadratic cone (5, 10), one sparse second-order cone (40, 10) and one LMI of order 6 over shared
    variables: the two big cones over all 62, the others over the first ten."""
    rng = np.random.default_rng(seed)
    sp = qs.make_cone(300, 62, ("tridiagonal", 2), "full", 0, point, rng)
    keep = np.zeros(sp["A"].shape, dtype=bool)
    for r in range(sp["A"].shape[0]):
        keep[r, rng.choice(62, 3, replace=False)] = True
    sp["A"] = np.where(keep, sp["A"], 0.0)
    big = km.make_cone("quad", 128, 62, "Q", point, rng)
    small = km.make_cone("quad", 5, 10, "Q", point, rng)
    so = km.make_cone("soc", 40, 10, None, point, rng)
    so["A"] = np.where(rng.uniform(0, 1, so["A"].shape) < 0.3, so["A"], 0.0)
    lmi = syn.lmi_problem(K=1, n=6, m=10, branching=1, overlap=1, seed=seed)
    return sp, big, small, so, (lmi["A"][0], lmi["C"][0], syn.scaling_points(1, 6, seed=seed + 1)[0])


def build_mixed(parts, with_sparse):
    sp, big, small, so, (A, Cm, Wl) = parts
    k = MixedContext(62, device=0)
    ids = {}
    if with_sparse:
        ids["sp"] = k.add_quadratic(sp["Q"], sp["A"].view(ByNonzeros), sp["c"], list(range(62)))
    ids["big"] = k.add_quadratic(big["Q"], big["A"], big["c"], list(range(62)))
    ids["small"] = k.add_quadratic(small["Q"], small["A"], small["c"], list(range(10)))
    ids["soc"] = k.add_soc_csr(*qs.csr_of(so["A"]), so["c"], list(range(10)))
    ids["lmi"] = k.add_lmi(A, Cm, list(range(10)))
    k.initialize()
    if with_sparse:
        k.set_W(ids["sp"], sp["W"])
    k.set_W(ids["big"], big["W"])
    k.set_W(ids["small"], small["W"])
    k.set_W(ids["soc"], so["W"])
    k.set_W(ids["lmi"], Wl)
    return k, ids


@pytest.mark.parametrize("point", km.POINTS, ids=POINT_IDS)
def test_mixed_context(point, monkeypatch):
    monkeypatch.setenv("CXK_STREAMED_QUADRATIC_MIN_WORK", str(MIXED_MIN_WORK))
    assert 5 * 5 + 6 * 10 < MIXED_MIN_WORK <= 128 * 128 + 129 * 62
    parts = mixed_problem(point, 91)
    sp, big, small, so, _ = parts
    k, ids = build_mixed(parts, True)
    alone, ids0 = build_mixed(parts, False)
    assert k.count_sparse_quadratic() == 1 and k.count_streamed_quadratic() == 2 and k.count_sparse_soc() == 1
    assert alone.count_sparse_quadratic() == 0 and alone.count_streamed_quadratic() == 1
    y = np.random.default_rng(92).uniform(-1, 1, 62)
    y *= 0.5 / max(km.slack_scale(sp, y), km.slack_scale(big, y), km.slack_scale(small, y[:10]), km.slack_scale(so, y[:10]))
    others = ("big", "small", "soc", "lmi")
    for ctx in (k, alone):
        ctx.assemble()
    G, AW, AQc, sc = k.constraint_schur(ids["sp"])
    r = km.ref_schur(sp)
    low = np.tril(np.ones_like(G, dtype=bool))
    km.within(G[low], r["G"][0][low], r["G"][1][low], km.C_SCHUR * r["g"], "G of the sparse cone")
    km.within(AW, *r["AW"], km.C_SCHUR, "AW of the sparse cone")
    km.within(AQc, *r["AQc"], km.C_SCHUR * r["g"], "AQc of the sparse cone")
    km.within(sc, *r["sc"], km.C_SCHUR * r["g"], "scalars of the sparse cone")
    for name in others:
        assert soc.same_bits(k.constraint_schur(ids[name]), alone.constraint_schur(ids0[name])), name
    k.prepare_step(y, km.C_WEIGHT, 1.0)
    alone.prepare_step(y, km.C_WEIGHT, 1.0)
    info, info0 = k.step_info(), alone.step_info()
    p = km.ref_prepare(sp, y)
    i, g = ids["sp"], p["g"]
    km.within(info[i, 0], *p["normsqrd"], km.C_PREPARE * g, "normsqrd of the sparse cone")
    km.within(info[i, 1], *p["norminfd"], km.C_PREPARE * g, "norminfd of the sparse cone")
    km.within(k.get_W(i), *p["wsqrt"], km.C_PREPARE * g, "w^1/2 of the sparse cone")
    for name in others:
        assert soc.same_bits(info[ids[name]], info0[ids0[name]]), name
    step = 0.5
    k.take_step(step, 1.0)
    alone.take_step(step, 1.0)
    Wn, Wm = km.ref_take(sp, y, step)
    km.within(k.get_W(i), Wn, Wm, km.C_TAKE * g, "W after the step of the sparse cone")
    for name in others:
        assert soc.same_bits(k.get_W(ids[name]), alone.get_W(ids0[name])), name


# ------------------------------------------------------------------------------------ refusals
def test_every_refusal_raises_with_its_message_and_the_context_stays_usable():
    k = host.check_refusals(0)
    assert k.count_sparse_quadratic() == 4 and k.count_structured_quadratic() == 2
    k.assemble()
    for i in range(4):
        assert np.all(np.isfinite(k.constraint_schur(i)[0]))
