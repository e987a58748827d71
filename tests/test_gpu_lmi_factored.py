"""LMIs given by factors (KktContext.add_lmi_factored, kernels_lmi_factored.hip.h) on the device.

Every row of lmi_factored_cases.ROWS runs at the three scaling points of test_gpu_lmi_kernel_matrix.py through the
stages of its run_point -- Schur complement, eigenvalue query, PrepareStep with step_info, TakeStep at the usual
step and at 1 / ||X||, the affine update -- against lmi_reference.py in longdouble on the expanded matrices, with
that file's constants and the magnitudes lmi_factored_cases.py describes.  The route is not one of the reported LMI
kernel instances, so run_point's lmi_kernels assertion has no counterpart here.  The oracle is built from the
expanded matrices.
"""
import numpy as np
import pytest

import lmi_factored_cases as fc
import lmi_reference as ref
import oracle_lib as ol
from conex_amd import KktContext
from conex_amd import synthetic as syn
from conex_amd.kkt import KktError
from test_gpu_lmi_kernel_matrix import (C_AFFINE, C_PREPARE, C_SCHUR, C_TAKE, C_WEIGHT, POINTS, TOL_LANCZOS, TOL_SPECTRUM,
                                        lanczos_determined, sample, within)
from test_gpu_parity import check_newton_step
from test_sharding import ThreadRanks, _newton_iteration

pytestmark = pytest.mark.gpu

POINT_IDS = [p if isinstance(p, str) else f"cond{p:.0e}" for p in POINTS]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def build_pair(prob, W):
    o = syn.build(ol.Program, prob, "lmi")  # (the expanded matrices)
    k = syn.build(KktContext, prob, "factored", device=0)
    for i in range(len(W)):
        o.set_W(i, W[i])
        k.set_W(i, W[i])
    return o, k


def run_point(prob, point, seed, lmax_exempt=False):
    K, n = len(prob["cliques"]), prob["n"]
    A, Cm = prob["A"], prob["C"]
    W = fc.points(prob, point, seed)
    o, k = build_pair(prob, W)
    assert k.count_factored_lmi() == K and k.count_lmi_kernel(3) == 0
    y = fc.direction(prob, seed)
    z = [y[cl] for cl in prob["cliques"]]
    picks = sample(K)

    # Schur complement
    k.assemble()
    for i in picks:
        r = fc.ref_schur(prob, i, W[i])
        Gk, AWk, AQk, sck = k.constraint_schur(i)
        low = np.tril(np.ones_like(Gk, dtype=bool))
        within(Gk[low], r["G"][0][low], r["G"][1][low], C_SCHUR, f"G of constraint {i}")
        within(AWk, *r["AW"], C_SCHUR, f"AW of constraint {i}")
        within(AQk, *r["AQc"], C_SCHUR, f"AQc of constraint {i}")
        within(sck, *r["sc"], C_SCHUR, f"<C, W>, <C, WCW> of constraint {i}")
        ptr = prob["rank_ptr"][i]
        for v in np.flatnonzero(np.diff(ptr) == 0):  # an empty variable: exact zeros
            assert not Gk[v, :v + 1].any() and not Gk[v:, v].any() and AWk[v] == 0.0 and AQk[v] == 0.0

    # the eigenvalue query
    ek = k.weighted_slack_eigenvalues(y, C_WEIGHT)
    eo = o.weighted_slack_eigenvalues(y, C_WEIGHT)
    preps = [fc.ref_prepare(prob, c, W[c], z[c]) for c in range(K)]
    within(ek[2], sum(p["frob"][0] for p in preps), sum(p["frob"][1] for p in preps), C_PREPARE, "query frob")
    within(ek[3], sum(p["trace"][0] for p in preps), sum(p["trace"][1] for p in preps), C_PREPARE, "query trace")
    spec = [ref.slack_spectrum(A[c], Cm[c], W[c], z[c], C_WEIGHT, 0) for c in range(K)]
    rho = max(max(abs(lo), abs(hi)) for lo, hi in spec)
    lo_all, hi_all = min(s[0] for s in spec), max(s[1] for s in spec)
    width = hi_all - lo_all
    # lmax, the converged end: always against the oracle, as in run_point -- but for fc.LMAX_EXEMPT
    if not lmax_exempt:
        assert abs(ek[1] - eo[1]) <= TOL_LANCZOS * rho, (ek, eo)
    else:
        # The device misses TOL_LANCZOS here.  The same expanded data through add_lmi (the large-order route) at the
        # same point, and the float64 recurrence's own movement of that Ritz value under one-ulp changes of WS: the
        # run is not determined by its input, and each implementation stays within twice that movement of the oracle.
        d = syn.build(KktContext, prob, "lmi", device=0)
        for i in range(K):
            d.set_W(i, W[i])
        ed = d.weighted_slack_eigenvalues(y, C_WEIGHT)
        spread = fc.dominant_end_spread(prob, W, z, spec)
        print(f"lmax against the oracle, of the spectral radius: factored {abs(ek[1] - eo[1]) / rho:.3g}, "
              f"expanded through add_lmi {abs(ed[1] - eo[1]) / rho:.3g}; one-ulp movement {spread / rho:.3g}")
        assert spread > TOL_LANCZOS * rho
        assert abs(ek[1] - eo[1]) <= 2 * spread and abs(ed[1] - eo[1]) <= 2 * spread, (ek, ed, eo, spread)
    assert ek[0] <= ek[1]
    stable_q, stable_p = lanczos_determined(A, Cm, W, z, 0, point, spec)
    if all(stable_q):
        assert -hi_all - TOL_SPECTRUM * rho <= ek[1] <= -lo_all + TOL_SPECTRUM * rho, (ek, spec)
        assert -hi_all - TOL_SPECTRUM * rho <= ek[0] <= -lo_all + TOL_SPECTRUM * rho, (ek, spec)
        assert abs(ek[0] - eo[0]) <= TOL_LANCZOS * max(width, np.finfo(float).tiny), (ek, eo)

    # PrepareStep, then TakeStep at the usual step and at one with ||X|| ~ 1
    WS1 = [np.asarray(ref.weighted_slack(A[c], Cm[c], W[c], z[c], C_WEIGHT, 0)[0], dtype=np.float64) for c in range(K)]
    xnorm = max(np.linalg.norm(ws[0] + np.eye(n), 2) for ws in WS1)
    for which in (0, 1):
        if which:
            for i in range(K):
                o.set_W(i, W[i])
                k.set_W(i, W[i])
        ik = k.prepare_step(y, C_WEIGHT, 1.0)
        io = o.prepare_step(y, C_WEIGHT, 1.0)
        info = k.step_info()
        for c in picks:
            within(info[c, 0], *preps[c]["normsqrd"], C_PREPARE, f"normsqrd of constraint {c}")
            if stable_p[c]:
                lo, hi = spec[c]
                assert info[c, 1] <= max(abs(1 + lo), abs(1 + hi)) + TOL_SPECTRUM * max(abs(lo), abs(hi))
        if all(stable_p):
            assert abs(ik[1] - io[1]) <= TOL_LANCZOS * max(width, abs(io[1])), (ik, io)
        step = min(1.0, 2.0 / ik[1] ** 2) if which == 0 else 1.0 / xnorm
        k.take_step(step, 1.0)
        for c in picks:
            Wn, Wm, growth = fc.ref_take_step(prob, c, W[c], z[c], 1.0, step)
            within(k.get_W(c).reshape(n, n), np.asarray(Wn).T, np.asarray(Wm).T, C_TAKE * growth,
                   f"W after the step {step:.3g} of constraint {c}")

    # the affine update
    for i in range(K):
        k.set_W(i, W[i])
    k.prepare_step(y, C_WEIGHT, 0.3, affine=1)
    for c in picks:
        Wa, Wm = fc.ref_affine(prob, c, W[c], z[c], 0.3)
        within(k.get_W(c).reshape(n, n), np.asarray(Wa).T, np.asarray(Wm).T, C_AFFINE, f"affine W of constraint {c}")


@pytest.mark.parametrize("point", POINTS, ids=POINT_IDS)
@pytest.mark.parametrize("row", list(fc.ROWS))
def test_factored_lmi_rows(row, point):
    run_point(fc.make_row(row), point, 31 + list(fc.ROWS).index(row), (row, point) in fc.LMAX_EXEMPT)


def test_the_lmax_exemption_names_one_point_of_the_rows():
    assert len(fc.LMAX_EXEMPT) == 1 and all(row in fc.ROWS and point in POINTS for row, point in fc.LMAX_EXEMPT)


def stages(prob, W, y):
    k = syn.build(KktContext, prob, "factored", device=0)
    for i in range(len(W)):
        k.set_W(i, W[i])
    k.assemble()
    out = [np.concatenate([np.ravel(np.tril(x)) if np.ndim(x) == 2 else np.ravel(x) for x in k.constraint_schur(i)])
           for i in range(len(W))]
    out.append(np.asarray(k.weighted_slack_eigenvalues(y, C_WEIGHT)))
    out.append(np.asarray(k.prepare_step(y, C_WEIGHT, 1.0)))
    k.take_step(0.5, 1.0)
    out += [k.get_W(i) for i in range(len(W))]
    return out


@pytest.mark.parametrize("row", ["n13-three-members", "n70-m40-R129", "n64-m65-rank1"])
def test_two_runs_give_the_same_bits(row):
    prob = fc.make_row(row)
    W = fc.points(prob, "well", 3)
    y = fc.direction(prob, 3)
    a, b = stages(prob, W, y), stages(prob, W, y)
    assert len(a) == len(b) and all(same_bits(x, z) for x, z in zip(a, b))


@pytest.mark.parametrize("row", ["n20-ranks-3-1-4-1-5-9", "n64-m65-rank1", "n70-m40-R129"])
def test_agrees_with_the_dense_route_on_the_expanded_data(row):
    """One context holding the factored constraint and its expansion (add_lmi) over the same variables, the same W:
    each is within the bound of the reference, so they are within twice the bound of each other."""
    prob = fc.make_row(row)
    W = fc.points(prob, "well", 4)[0]
    m = prob["m"]
    k = KktContext(m, device=0)
    assert k.add_lmi_factored(prob["F"][0], prob["rank_ptr"][0], prob["sigma"][0], prob["C"][0], list(range(m))) == 0
    assert k.add_lmi(prob["A"][0], prob["C"][0], list(range(m))) == 1
    k.initialize()
    assert k.count_factored_lmi() == 1
    assert "schur" in k.lmi_kernels(1)
    with pytest.raises(KktError):
        k.lmi_kernels(0)
    k.set_W(0, W)
    k.set_W(1, W)
    k.assemble()
    r = fc.ref_schur(prob, 0, W)
    f, d = k.constraint_schur(0), k.constraint_schur(1)
    low = np.tril(np.ones((m, m), dtype=bool))
    for got, want, key in ((f[0][low], d[0][low], "G"), (f[1], d[1], "AW"), (f[2], d[2], "AQc")):
        mag = r[key][1][low] if key == "G" else r[key][1]
        assert np.all(np.abs(got - want) <= 2 * C_SCHUR * ref.U64 * np.asarray(mag, dtype=np.float64)), key


@pytest.mark.parametrize("row", ["n13-three-members", "n64-m65-rank1"])
def test_prepare_take_step_equals_prepare_then_take(row):
    prob = fc.make_row(row)
    W = fc.points(prob, "well", 5)
    y = fc.direction(prob, 5)
    ws = []
    for fused in (True, False):
        k = syn.build(KktContext, prob, "factored", device=0)
        for i in range(len(W)):
            k.set_W(i, W[i])
        if fused:
            n2, ninf, took = k.prepare_take_step(y, C_WEIGHT, 1.0)
            assert not took  # (the large-order step argument takes the step length from the host)
        else:
            n2, ninf = k.prepare_step(y, C_WEIGHT, 1.0)
        k.take_step(min(1.0, 2.0 / ninf ** 2), 1.0)
        ws.append([np.r_[n2, ninf]] + [k.get_W(i) for i in range(len(W))])
    assert all(same_bits(a, b) for a, b in zip(*ws))


def mixed_program():
    """A factored cone (order 12, ranks 1 and 2), a dense LMI of order 20, a second-order cone and a linear block on
    one clique tree of four cliques of 8 variables."""
    rng = np.random.default_rng(17)
    cliques, num_vars = syn.tree_cliques(4, 2, 8, 2)
    fp = syn.factored_lmi_problem(K=1, n=12, ranks=(1, 2, 1, 1, 2, 1, 1, 1), seed=18)
    A20 = np.stack([syn.random_sym(rng, 20) for _ in range(8)])
    As = rng.uniform(-1, 1, (11, 8))
    cs = np.r_[1.0, np.zeros(10)]
    Al = rng.uniform(-1, 1, (15, 8))
    cl = np.abs(rng.uniform(0.5, 1.5, 15))
    b = rng.uniform(-1, 1, num_vars) * 0.1

    def build(p, factored):
        if factored:
            assert p.add_lmi_factored(fp["F"][0], fp["rank_ptr"][0], fp["sigma"][0], fp["C"][0], cliques[0]) == 0
        else:
            assert p.add_lmi(fp["A"][0], fp["C"][0], cliques[0]) == 0
        assert p.add_lmi(A20, np.eye(20), cliques[1]) == 1
        assert p.add_soc(As, cs, cliques[2]) == 2
        assert p.add_linear(Al, cl, cliques[3]) == 3
        p.initialize()
        return p

    W = [syn.scaling_points(1, 12, seed=19)[0], syn.scaling_points(1, 20, seed=20)[0], syn.soc_scaling_points(1, 10, seed=21)[0],
         rng.uniform(0.5, 1.5, 15)]
    return build, W, b, num_vars


def test_mixed_context_against_the_oracle():
    build, W, b, num_vars = mixed_program()
    o = build(ol.Program(num_vars), False)
    k = build(KktContext(num_vars, device=0), True)
    for i, w in enumerate(W):
        o.set_W(i, w)
        k.set_W(i, w)
    assert k.count_factored_lmi() == 1
    assert k.L.cxk_device_mu_supported(k.h) == 0 and k.L.cxk_triple_supported(k.h) == 0
    assert not k.fused_assembly() and not k.fused_tree()
    assert sum(k.count_lmi_kernel(w) for w in range(5)) == 1  # the order-20 LMI alone
    check_newton_step(o, k, b, lanczos_tol=1e-6)


def test_line_search_refuses_and_the_device_iteration_is_off():
    prob = fc.make_row("n20-ranks-3-1-4-1-5-9")
    k = syn.build(KktContext, prob, "factored", device=0)
    assert k.L.cxk_device_mu_supported(k.h) == 0 and k.L.cxk_triple_supported(k.h) == 0
    assert not k.fused_assembly() and not k.fused_tree()
    plain = syn.build(KktContext, prob, "lmi", device=0)
    k.set_cost(prob["b"])
    plain.set_cost(prob["b"])
    assert k.kkt_solve(prob["b"], 0.7)[0] == 1 and plain.kkt_solve(prob["b"], 0.7)[0] == 1
    assert k.line_search(10.0) == -1.0 and plain.line_search(10.0) == -1.0  # (as every non-linear cone)
    byt, flops = k.assembly_work()
    byt0, flops0 = plain.assembly_work()
    assert 0 < flops and 0 < byt and (byt, flops) != (byt0, flops0)


def test_counts_with_other_groups_in_the_context():
    """Two groups of factored cones (R = 3 and R = 4 at equal n, m), a dense LMI and a linear block."""
    rng = np.random.default_rng(23)
    k = KktContext(3, device=0)
    C = np.eye(6)
    for ranks in ((1, 1, 1), (1, 2, 1), (2, 1, 1), (0, 2, 1)):
        R = sum(ranks)
        k.add_lmi_factored(rng.standard_normal((6, R)), np.r_[0, np.cumsum(ranks)], None, C)
    k.add_lmi(np.stack([syn.random_sym(rng, 6) for _ in range(3)]), C)
    k.add_linear(rng.uniform(-1, 1, (4, 3)), np.ones(4))
    k.initialize()
    assert k.count_factored_lmi() == 4
    assert sum(k.count_lmi_kernel(w) for w in range(5)) == 1
    for i in range(4):
        with pytest.raises(KktError):
            k.lmi_kernels(i)
    assert set(k.lmi_kernels(4)) == {"schur", "prepare", "query", "take", "affine"}
    k.assemble()
    assert all(np.all(np.isfinite(k.constraint_schur(i)[0])) for i in range(5))


def test_sharded_direction_with_factored_cones_equals_the_unsharded_one():
    """World 2 (the thread ranks and host all-reduce of test_sharding.py) on a clique tree of factored cones: one
    Newton iteration equals the single context's to that file's tolerance."""
    K, world = 12, 2
    prob = syn.factored_lmi_problem(K=K, n=9, ranks=(1, 2, 1, 1, 1, 2), branching=2, overlap=2, seed=41)
    W = syn.scaling_points(K, 9, seed=42)
    single = syn.build(KktContext, prob, "factored", device=0)
    assert single.count_factored_lmi() == K
    want = _newton_iteration(single, prob, W, False)

    def body(rank, allreduce):
        k = KktContext(prob["num_vars"], device=0)
        for i, cl in enumerate(prob["cliques"]):
            assert k.add_lmi_factored(prob["F"][i], prob["rank_ptr"][i], prob["sigma"][i], prob["C"][i], cl) == i
        k.set_shard(rank, world)
        k.initialize()
        k.comm_set_allreduce(allreduce)
        k.set_cost(prob["b"])
        out = _newton_iteration(k, prob, W, True)
        out["factored"] = k.count_factored_lmi()
        return out

    outs = ThreadRanks(world).run(body)
    assert all(0 < out["factored"] < K for out in outs) and sum(out["factored"] for out in outs) >= K
    for out in outs:
        for key in ("y", "y2", "y3"):
            assert np.linalg.norm(out[key] - want[key]) <= 1e-10 * np.linalg.norm(want[key]), key
        assert np.allclose(out["eig"], want["eig"], rtol=1e-9, atol=0)
        assert np.allclose(out["info"], want["info"], rtol=1e-9, atol=0)
        for i, w in out["W"].items():
            assert np.linalg.norm(w - want["W"][i]) <= 1e-10 * np.linalg.norm(want["W"][i])
