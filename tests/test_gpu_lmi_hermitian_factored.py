"""Hermitian matrix inequalities over R / C / H given by factors (KktContext.add_hermitian_factored,
kernels_lmi_factored.hip.h) on the device.

Every row of lmi_hermitian_factored_cases.ROWS runs at the three scaling points of test_gpu_lmi_kernel_matrix.py
through the stages of test_gpu_lmi_factored.run_point -- Schur complement, eigenvalue query, PrepareStep with
step_info, TakeStep at the usual step and at 1 / ||X||, the affine update -- against lmi_reference.py with its d
argument in longdouble on the expanded planes, with that file's constants and the magnitudes
lmi_hermitian_factored_cases.py describes.  The oracle is built from the expanded planes (add_hermitian).
"""
import numpy as np
import pytest

import lmi_hermitian_factored_cases as hc
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
    o = syn.build(ol.Program, prob, "herm")  # (the expanded planes)
    k = syn.build(KktContext, prob, "herm-factored", device=0)
    for i in range(len(W)):
        o.set_W(i, W[i])
        k.set_W(i, W[i])
    return o, k


def run_point(prob, point, seed):
    K, n, d = len(prob["cliques"]), prob["n"], prob["d"]
    A, Cm = prob["A"], prob["C"]
    W = hc.points(prob, point, seed)
    o, k = build_pair(prob, W)
    assert k.count_factored_lmi() == K and k.count_lmi_kernel(3) == 0
    y = hc.direction(prob, seed)
    z = [y[cl] for cl in prob["cliques"]]
    picks = sample(K)

    # Schur complement
    k.assemble()
    for i in picks:
        r = hc.ref_schur(prob, i, W[i])
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
    preps = [hc.ref_prepare(prob, c, W[c], z[c]) for c in range(K)]
    within(ek[2], sum(p["frob"][0] for p in preps), sum(p["frob"][1] for p in preps), C_PREPARE, "query frob")
    within(ek[3], sum(p["trace"][0] for p in preps), sum(p["trace"][1] for p in preps), C_PREPARE, "query trace")
    spec = [ref.slack_spectrum(A[c], Cm[c], W[c], z[c], C_WEIGHT, d) for c in range(K)]
    rho = max(max(abs(lo), abs(hi)) for lo, hi in spec)
    lo_all, hi_all = min(s[0] for s in spec), max(s[1] for s in spec)
    width = hi_all - lo_all
    # lmax, the converged end: always against the oracle, as in run_point (no row and point is exempt:
    # hc.LMAX_EXEMPT is empty, measured at most 8e-16 of the spectral radius)
    print(f"lmax against the oracle, of the spectral radius: {abs(ek[1] - eo[1]) / rho:.3g}")
    assert abs(ek[1] - eo[1]) <= TOL_LANCZOS * rho, (ek, eo)
    assert ek[0] <= ek[1]
    stable_q, stable_p = lanczos_determined(A, Cm, W, z, d, point, spec)
    if all(stable_q):
        assert -hi_all - TOL_SPECTRUM * rho <= ek[1] <= -lo_all + TOL_SPECTRUM * rho, (ek, spec)
        assert -hi_all - TOL_SPECTRUM * rho <= ek[0] <= -lo_all + TOL_SPECTRUM * rho, (ek, spec)
        # (a single cone of order 1 has one eigenvalue: lmin is the converged end, and lmax's bound is its bound)
        assert abs(ek[0] - eo[0]) <= TOL_LANCZOS * (width if width > 0 else rho), (ek, eo)

    # PrepareStep, then TakeStep at the usual step and at one with ||X|| ~ 1
    WS1 = [np.asarray(ref.weighted_slack(A[c], Cm[c], W[c], z[c], C_WEIGHT, d)[0], dtype=np.float64) for c in range(K)]
    for ws in WS1:
        ws[0] += np.eye(n)
    xnorm = max(np.linalg.norm(ref.complex_rep(ws, d), 2) for ws in WS1)
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
            Wn, Wm, growth = hc.ref_take_step(prob, c, W[c], z[c], 1.0, step)
            within(k.get_W(c).reshape(np.shape(Wn)), np.asarray(Wn), np.asarray(Wm), C_TAKE * growth,
                   f"W after the step {step:.3g} of constraint {c}")

    # the affine update
    for i in range(K):
        k.set_W(i, W[i])
    k.prepare_step(y, C_WEIGHT, 0.3, affine=1)
    for c in picks:
        Wa, Wm = hc.ref_affine(prob, c, W[c], z[c], 0.3)
        within(k.get_W(c).reshape(np.shape(Wa)), np.asarray(Wa), np.asarray(Wm), C_AFFINE, f"affine W of constraint {c}")


@pytest.mark.parametrize("point", POINTS, ids=POINT_IDS)
@pytest.mark.parametrize("row", list(hc.ROWS))
def test_factored_hermitian_rows(row, point):
    run_point(hc.make_row(row), point, hc.row_seed(row))


def test_the_lmax_exemptions_are_at_most_one_point_per_d():
    assert len(hc.LMAX_EXEMPT) == 0
    assert all(row in hc.ROWS and point in POINTS for row, point in hc.LMAX_EXEMPT)
    for d in (1, 2, 4):
        assert sum(hc.ROWS[row]["d"] == d for row, _ in hc.LMAX_EXEMPT) <= 1


def stages(prob, W, y):
    k = syn.build(KktContext, prob, "herm-factored", device=0)
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


@pytest.mark.parametrize("row", ["n7-three-members-d2", "n8-R65-d4", "n6-m17-rank1-d2"])
def test_two_runs_give_the_same_bits(row):
    prob = hc.make_row(row)
    W = hc.points(prob, "well", 3)
    y = hc.direction(prob, 3)
    a, b = stages(prob, W, y), stages(prob, W, y)
    assert len(a) == len(b) and all(same_bits(x, z) for x, z in zip(a, b))


@pytest.mark.parametrize("row", ["n5-ranks-3-1-0-2-d2", "n6-m17-rank1-d4", "n8-R65-d2", "n9-d1"])
def test_agrees_with_add_hermitian_on_the_expanded_planes(row):
    """One context holding the factored constraint and its expansion (add_hermitian) over the same variables, the same
    W: each is within the bound of the reference, so they are within twice the bound of each other."""
    prob = hc.make_row(row)
    W = hc.points(prob, "well", 4)[0]
    m = prob["m"]
    k = KktContext(m, device=0)
    assert k.add_hermitian_factored(prob["F"][0], prob["rank_ptr"][0], prob["sigma"][0], prob["C"][0], list(range(m))) == 0
    assert k.add_hermitian(prob["A"][0], prob["C"][0], list(range(m))) == 1
    k.initialize()
    assert k.count_factored_lmi() == 1
    assert "schur" in k.lmi_kernels(1)
    with pytest.raises(KktError):
        k.lmi_kernels(0)
    k.set_W(0, W)
    k.set_W(1, W)
    k.assemble()
    r = hc.ref_schur(prob, 0, W)
    f, dn = k.constraint_schur(0), k.constraint_schur(1)
    low = np.tril(np.ones((m, m), dtype=bool))
    for got, want, key in ((f[0][low], dn[0][low], "G"), (f[1], dn[1], "AW"), (f[2], dn[2], "AQc"), (f[3], dn[3], "sc")):
        mag = r[key][1][low] if key == "G" else r[key][1]
        assert np.all(np.abs(got - want) <= 2 * C_SCHUR * ref.U64 * np.asarray(mag, dtype=np.float64)), key


@pytest.mark.parametrize("row", ["n7-three-members-d4", "n6-m17-rank1-d2"])
def test_prepare_take_step_equals_prepare_then_take(row):
    prob = hc.make_row(row)
    W = hc.points(prob, "well", 5)
    y = hc.direction(prob, 5)
    ws = []
    for fused in (True, False):
        k = syn.build(KktContext, prob, "herm-factored", device=0)
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
    """A factored complex cone (order 6, ranks 1 and 2), a dense quaternion cone of order 3, a second-order cone and a
    linear block on one clique tree of four cliques of 8 variables."""
    rng = np.random.default_rng(17)
    cliques, num_vars = syn.tree_cliques(4, 2, 8, 2)
    fp = syn.factored_hermitian_problem(K=1, n=6, d=2, ranks=(1, 2, 1, 1, 2, 1, 1, 1), signs="mixed", seed=18)
    Ah = np.stack([syn.random_hermitian(rng, 4, 3) for _ in range(8)])
    Ch = np.zeros((4, 3, 3))
    Ch[0] = np.eye(3)
    As = rng.uniform(-1, 1, (11, 8))
    cs = np.r_[1.0, np.zeros(10)]
    Al = rng.uniform(-1, 1, (15, 8))
    cl = np.abs(rng.uniform(0.5, 1.5, 15))
    b = rng.uniform(-1, 1, num_vars) * 0.1

    def build(p, factored):
        if factored:
            assert p.add_hermitian_factored(fp["F"][0], fp["rank_ptr"][0], fp["sigma"][0], fp["C"][0], cliques[0]) == 0
        else:
            assert p.add_hermitian(fp["A"][0], fp["C"][0], cliques[0]) == 0
        assert p.add_hermitian(Ah, Ch, cliques[1]) == 1
        assert p.add_soc(As, cs, cliques[2]) == 2
        assert p.add_linear(Al, cl, cliques[3]) == 3
        p.initialize()
        return p

    W = [syn.hermitian_scaling_points(1, 6, 2, seed=19)[0], syn.hermitian_scaling_points(1, 3, 4, seed=20)[0],
         syn.soc_scaling_points(1, 10, seed=21)[0], rng.uniform(0.5, 1.5, 15)]
    return build, W, b, num_vars


def test_mixed_context_against_the_oracle():
    build, W, b, num_vars = mixed_program()
    o = build(ol.Program(num_vars), False)
    k = build(KktContext(num_vars, device=0), True)
    for i, w in enumerate(W):
        o.set_W(i, w)
        k.set_W(i, w)
    assert k.count_factored_lmi() == 1
    assert sum(k.count_lmi_kernel(w) for w in range(5)) == 1  # the dense quaternion cone alone
    check_newton_step(o, k, b, lanczos_tol=1e-6)


def test_the_device_iteration_and_the_fused_launches_report_off():
    prob = hc.make_row("n6-m17-rank1-d2")  # (a row without an empty variable: its Schur complement is definite)
    k = syn.build(KktContext, prob, "herm-factored", device=0)
    assert k.L.cxk_device_mu_supported(k.h) == 0 and k.L.cxk_triple_supported(k.h) == 0
    assert not k.fused_assembly() and not k.fused_tree()
    plain = syn.build(KktContext, prob, "herm", device=0)
    k.set_cost(prob["b"])
    plain.set_cost(prob["b"])
    assert k.kkt_solve(prob["b"], 0.7)[0] == 1 and plain.kkt_solve(prob["b"], 0.7)[0] == 1
    assert k.line_search(10.0) == -1.0 and plain.line_search(10.0) == -1.0  # (as every non-linear cone)
    byt, flops = k.assembly_work()
    byt0, flops0 = plain.assembly_work()
    assert 0 < flops and 0 < byt and (byt, flops) != (byt0, flops0)


def test_sharded_direction_with_factored_hermitian_cones_equals_the_unsharded_one():
    """World 2 (the thread ranks and host all-reduce of test_sharding.py) on a clique tree of factored complex cones: one
    Newton iteration equals the single context's to that file's tolerance."""
    K, world = 12, 2
    prob = syn.factored_hermitian_problem(K=K, n=5, d=2, ranks=(1, 2, 1, 1, 1, 2), branching=2, overlap=2, seed=41)
    W = syn.hermitian_scaling_points(K, 5, 2, seed=42)
    single = syn.build(KktContext, prob, "herm-factored", device=0)
    assert single.count_factored_lmi() == K
    want = _newton_iteration(single, prob, W, False)

    def body(rank, allreduce):
        k = KktContext(prob["num_vars"], device=0)
        for i, cl in enumerate(prob["cliques"]):
            assert k.add_hermitian_factored(prob["F"][i], prob["rank_ptr"][i], prob["sigma"][i], prob["C"][i], cl) == i
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
