"""Sharded contexts (cxk_set_shard, world > 1) must take the same branch on every rank at every failure.

A rank that reports a failed factorization while the others report success leaves the interior-point loop
early, and the others then wait in a collective that never completes: with RCCL a hang of every rank.
The ranks here are threads of one process (ThreadRanks, test_sharding.py): a rank that parts ways makes
the barrier of the all-reduce time out and the test fail instead of hang.

  * time-outs of the whole-tree launches, faked on ONE rank by cxk_debug_fused_timeout_at (it writes the
    two words a wait that ran out writes, nothing else): one before the exchange (kFusedShardUp), one
    behind it (kFusedShardTop).  Every rank must report the same ok from cxk_factor_status and cxk_sync
    and the same cxk_fused_tree_timed_out, and the next step must succeed everywhere;
  * failed pivots in the replicated top, below the cut on the level kernels, and on the sharded LDLT path;
  * whole CONEX_Maximize runs with a time-out on one rank.

Every y a rank reports good is held against a float64 dense solve of the same system, assembled by the
oracle (oracle/), at relative error <= 1e-10.
"""
import numpy as np
import pytest

import oracle_lib as ol
from conex_amd import KktContext
from conex_amd import synthetic as syn
from test_sharding import ThreadRanks, _maximize, _program

pytestmark = pytest.mark.gpu

TOL = 1e-10
BUILD_KIND = {"c4": "lmi", "mixed": "mixed", "chain": "soc"}
# (inv_sqrt_mu, b_scaling, c_scaling) of the steps: a new right-hand side each, so a stale y is caught
STEPS = [(0.7, 0.9, 0.8), (0.6, 1.1, 0.7), (0.8, 0.5, 1.2), (0.9, 1.0, 1.0)]
SITES = {"shard-up": KktContext.DEBUG_FUSED_SHARD_UP, "shard-top": KktContext.DEBUG_FUSED_SHARD_TOP}

_REFS = {}


def _reference(kind):
    """float64 dense solves of the system every step assembles (same W, same b): y per step."""
    if kind not in _REFS:
        prob, W = _program(kind, 11)
        o = syn.build(ol.Program, prob, BUILD_KIND[kind])
        for i in range(len(prob["cliques"])):
            o.set_W(i, W[i])
        o.assemble()
        AW, AQc, _ = o.residuals()
        K = o.kkt_matrix()
        b = np.asarray(prob["b"], dtype=np.float64)
        _REFS[kind] = [np.linalg.solve(K, kk * bs * b + kk * cs * AQc - 2.0 * AW) for kk, bs, cs in STEPS]
    return _REFS[kind]


def _rank_context(prob, kind, rank, world, allreduce, W=None):
    k = KktContext(prob["num_vars"], device=0)
    for c, cl in enumerate(prob["cliques"]):
        if kind == "c4":
            k.add_lmi(prob["A"][c], prob["C"][c], cl)
        elif kind == "chain":
            k.add_soc(prob["A"][c], prob["c"][c], cl)
        elif prob["kinds"][c] == "herm":
            k.add_hermitian(prob["A"][c], prob["C"][c], cl)
        else:
            k.add_soc(prob["A"][c], prob["C"][c], cl)
    k.set_shard(rank, world)
    k.initialize()
    k.comm_set_allreduce(allreduce)
    k.set_cost(prob["b"])
    if W is not None:
        for i in range(k.K):
            if k.owns(i):
                k.set_W(i, W[i])
    return k


def _step(k, kk, bs, cs):
    """One factor-and-solve; what every rank must agree on, and the y it reads back."""
    k.kkt_solve_async(kk, bs, cs)
    status = k.factor_status()
    ok = k.sync()
    return {"status": status, "sync": ok, "y": k.get_y(), "timed_out": k.fused_tree_timed_out(),
            "fused": k.fused_tree()}


def _agree(res, step, key):
    vals = [r[step][key] for r in res]
    assert len(set(vals)) == 1, f"step {step}: ranks disagree on {key}: {vals}"
    return vals[0]


def _check_good_y(res, ref):
    for rank, steps in enumerate(res):
        for s, out in enumerate(steps):
            if out["status"] and out["sync"]:
                err = np.linalg.norm(out["y"] - ref[s]) / np.linalg.norm(ref[s])
                assert err <= TOL, f"rank {rank} step {s}: y reported good, relative error {err:.3e}"


@pytest.mark.parametrize("world", [2, 3, 4])
@pytest.mark.parametrize("victim", ["first", "last"])
@pytest.mark.parametrize("site", list(SITES))
@pytest.mark.parametrize("kind", ["c4", "mixed", "chain"])
def test_a_timeout_on_one_rank_is_settled_alike_on_every_rank(monkeypatch, kind, site, victim, world):
    """good step, the hook fires on the victim, two more steps.  A time-out before the exchange travels
    with it: every rank reports the failure and the time-out, and every rank goes over to the level
    kernels.  One behind the exchange is known to the victim only: it redoes its part locally and every
    rank reports success.  (Level-kernel contexts, CXK_NO_FUSED_TREE, make no whole-tree launch: the hook
    is refused there, see test_the_hook_is_refused_where_it_cannot_fire.)"""
    monkeypatch.delenv("CXK_NO_FUSED_TREE", raising=False)
    monkeypatch.delenv("CXK_NO_FUSED_SHARD", raising=False)
    prob, W = _program(kind, 11)
    ref = _reference(kind)
    v = 0 if victim == "first" else world - 1

    def body(rank, allreduce):
        k = _rank_context(prob, kind, rank, world, allreduce, W)
        assert k.fused_tree()
        out = [_step(k, *STEPS[0])]
        if rank == v:
            k.debug_fused_timeout_at(0, SITES[site])
        out += [_step(k, *s) for s in STEPS[1:]]
        return out

    res = ThreadRanks(world).run(body)
    for s in range(len(STEPS)):
        status = _agree(res, s, "status")
        assert _agree(res, s, "sync") == status
        timed_out = _agree(res, s, "timed_out")
        if s == 1 and site == "shard-up":
            assert status == 0 and timed_out, "a time-out before the exchange is a failure every rank reports"
        else:
            assert status == 1 and not timed_out, f"step {s}"
    # the hook fired: the ranks that learnt of it sweep level by level from then on
    fused_after = [r[1]["fused"] for r in res]
    if site == "shard-up":
        assert not any(fused_after)
    else:
        assert fused_after == [r != v for r in range(world)]
    _check_good_y(res, ref)


@pytest.mark.parametrize("level", [False, True])
def test_the_hook_is_refused_where_it_cannot_fire(monkeypatch, level):
    """A sharded context makes no single-GPU factor launch, and with CXK_NO_FUSED_TREE no whole-tree
    launch at all: the hook must not arm silently (a time-out test would then pass without one)."""
    if level:
        monkeypatch.setenv("CXK_NO_FUSED_TREE", "1")
    else:
        monkeypatch.delenv("CXK_NO_FUSED_TREE", raising=False)
    prob, W = _program("c4", 11)

    def body(rank, allreduce):
        k = _rank_context(prob, "c4", rank, 2, allreduce)
        refused = []
        for site in (KktContext.DEBUG_FUSED_FACTOR, KktContext.DEBUG_FUSED_SHARD_UP, KktContext.DEBUG_FUSED_SHARD_TOP):
            try:
                k.debug_fused_timeout_at(0, site)
                refused.append(False)
            except Exception:  # noqa: BLE001 -- KktError
                refused.append(True)
        return refused

    for refused in ThreadRanks(2).run(body):
        assert refused == ([True, True, True] if level else [True, False, False])


def _three_steps(res, ref, bad_ok):
    """good, bad, good again: every rank agrees at each step."""
    for s, want in enumerate([1, bad_ok, 1]):
        status = _agree(res, s, "status")
        assert _agree(res, s, "sync") == status == want, f"step {s}"
        assert not _agree(res, s, "timed_out")
    for rank, steps in enumerate(res):
        for s in (0, 2):
            err = np.linalg.norm(steps[s]["y"] - ref[s]) / np.linalg.norm(ref[s])
            assert err <= TOL, f"rank {rank} step {s}: relative error {err:.3e}"


@pytest.mark.parametrize("world", [2, 3, 4])
@pytest.mark.parametrize("fused", [True, False])
def test_a_failed_pivot_in_the_replicated_top_is_seen_by_every_rank(monkeypatch, fused, world):
    """An indefinite scaling point (W = 1e3 diag(1, -1, ...)) makes the Schur block of a constraint of the
    top indefinite, 1e6 times larger than the rest: the top's factorization fails.  The top is factored by
    every rank after the all-reduce (one rank assembled the constraint) -- on the whole-tree kernels and
    on the level kernels."""
    if fused:
        monkeypatch.delenv("CXK_NO_FUSED_TREE", raising=False)
    else:
        monkeypatch.setenv("CXK_NO_FUSED_TREE", "1")
    monkeypatch.delenv("CXK_NO_FUSED_SHARD", raising=False)
    prob, W = _program("c4", 11)
    ref = _reference("c4")
    Wbad = 1e3 * np.diag([1.0 if j % 2 == 0 else -1.0 for j in range(20)])

    def body(rank, allreduce):
        k = _rank_context(prob, "c4", rank, world, allreduce, W)
        assert k.fused_tree() == fused
        return k, k.valid_variables()

    # which constraints lie in the top: their whole clique is valid on every rank
    def run(rank, allreduce):
        k, valid = body(rank, allreduce)
        everywhere = np.asarray(allreduce(valid.astype(np.float64), 2)) > 0   # min over the ranks
        top = [i for i, cl in enumerate(prob["cliques"]) if np.all(everywhere[cl])]
        assert top, "the cut leaves a replicated top"
        bad = top[-1]
        out = [_step(k, *STEPS[0])]
        if k.owns(bad):
            k.set_W(bad, Wbad)
        out.append(_step(k, *STEPS[1]))
        if k.owns(bad):
            k.set_W(bad, W[bad])
        out.append(_step(k, *STEPS[2]))
        return [dict(o, owner=bool(k.owns(bad))) for o in out]

    res = ThreadRanks(world).run(run)
    assert sum(r[0]["owner"] for r in res) == 1
    _three_steps(res, ref, 0)


@pytest.mark.parametrize("world", [2, 3, 4])
def test_a_failed_pivot_below_the_cut_on_the_level_kernels_is_seen_by_every_rank(monkeypatch, world):
    """test_a_failed_leaf_pivot_on_one_rank_is_seen_by_every_rank on the level kernels (CXK_NO_FUSED_TREE):
    the failure is fail[0] of the rank that owns the leaf, and travels in exchange_pack's failure word."""
    monkeypatch.setenv("CXK_NO_FUSED_TREE", "1")
    prob, W = _program("c4", 11)
    ref = _reference("c4")
    bad = len(prob["cliques"]) - 1                # a leaf of the clique tree

    def body(rank, allreduce):
        k = _rank_context(prob, "c4", rank, world, allreduce, W)
        assert not k.fused_tree()
        everywhere = np.asarray(allreduce(k.valid_variables().astype(np.float64), 2)) > 0   # min over the ranks
        assert not np.all(everywhere[prob["cliques"][bad]]), "the leaf lies below the cut"
        out = [_step(k, *STEPS[0])]
        if k.owns(bad):
            k.set_W(bad, np.zeros((20, 20)))
        out.append(_step(k, *STEPS[1]))
        if k.owns(bad):
            k.set_W(bad, W[bad])
        out.append(_step(k, *STEPS[2]))
        return [dict(o, owner=bool(k.owns(bad))) for o in out]

    res = ThreadRanks(world).run(body)
    assert sum(r[0]["owner"] for r in res) == 1
    _three_steps(res, ref, 0)


def test_a_singular_block_on_the_sharded_ldlt_path_is_settled_alike():
    """Equality constraints (the LQR program of test_sharded_equality_constraints_take_the_ldlt_path): one
    rank's part of the assembled matrix is zeroed, so its subtrees' pivots are all zero.  The block LDLT
    has no failing factorization: it clamps such pivots to +-1e-9 and reports success, as the reference's
    RLDLT does (kernels_tree_level.hip.h, tree_sweep_block_ldlt).  So what is checked is that every rank reports
    the same outcome of the singular factorization, and that the next factorization of the real matrix
    solves like a float64 dense solve of the oracle's assembled matrix."""
    from test_oracle_kat import build_lqr_problem
    world, victim = 3, 1
    o = build_lqr_problem(ol.Program, 40)
    o.assemble()
    rhs = np.random.default_rng(2).uniform(-1, 1, o.N)
    y_ref = np.linalg.solve(o.kkt_matrix(), rhs)

    def _sharded(nv, rank):
        k = KktContext(nv, device=0)
        k.set_shard(rank, world)
        return k

    def body(rank, allreduce):
        k = build_lqr_problem(lambda nv, **kw: _sharded(nv, rank), 40)
        k.comm_set_allreduce(allreduce)
        out = []
        for bad in (False, True, False):
            k.assemble()
            if bad and rank == victim:
                k.set_slab(np.zeros(k.slab_size()))
            ok = k.factor()
            y = k.solve_inplace(rhs)
            out.append({"status": k.factor_status(), "sync": ok, "timed_out": k.fused_tree_timed_out(), "y": y})
        return out

    res = ThreadRanks(world).run(body)
    for s in range(3):
        status = _agree(res, s, "status")
        assert _agree(res, s, "sync") == status == 1
        assert not _agree(res, s, "timed_out")
    for steps in res:
        for s in (0, 2):
            err = np.linalg.norm(steps[s]["y"] - y_ref) / np.linalg.norm(y_ref)
            assert err <= TOL, f"step {s}: relative error {err:.3e}"


@pytest.mark.parametrize("site", list(SITES) + ["shard-top-stream-ordered"])
def test_sharded_conex_maximize_with_a_timeout_on_one_rank(capfd, site):
    """CONEX_Maximize at world 3; the whole-tree factor launch of iteration 2 of rank 1 reports a time-out.
    Every rank must finish with the same status and iteration count, at the single-GPU optimum."""
    prob = syn.lmi_problem(K=100, n=20, m=20, branching=8, overlap=5, seed=21)
    ok0, y0, it0 = _maximize(prob, 0, 1, None)
    assert ok0 == 1
    world, victim = 3, 1
    capfd.readouterr()
    which = SITES.get(site, KktContext.DEBUG_FUSED_SHARD_TOP | KktContext.DEBUG_FUSED_STREAM_ORDERED)
    results = ThreadRanks(world).run(
        lambda r, ar: _maximize(prob, r, world, ar, hook=(2, which) if r == victim else None))
    notes = capfd.readouterr().err.count("a wait inside the whole-tree launch ran out")
    # shard-up: every rank learns of it from the exchange.  shard-top: the victim redoes it alone -- or, when
    # the host word is raised only after the mu selection's reduction went out, every rank learns of it there
    want = {"shard-up": (world,), "shard-top": (1,)}.get(site, (1, world))
    assert notes in want, f"the time-out was settled by {notes} ranks"
    its = [it for _, _, it in results]
    assert len(set(its)) == 1, its
    for ok, y, it in results:
        assert ok == 1 and abs(it - it0) <= 3
        assert np.array_equal(y, results[0][1])           # every rank returns the same vector
        assert abs(prob["b"] @ y - prob["b"] @ y0) <= 1e-6 * abs(prob["b"] @ y0)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("between", ["eigenvalues", "solve"])
def test_a_top_timeout_with_work_behind_it_reaches_every_rank(monkeypatch, between, world):
    """The host word of a top launch's time-out is raised by a host function on the stream, as a launch still
    running when the host goes on would raise it.  An eigenvalue query or a solve sweep goes out between the
    launch and cxk_factor_status, as in the interior-point loop's mu selection.  Either the victim saw the word
    before that (it redoes the launch alone, before anything used it: every rank succeeds and the query is
    right), or the query carried the time-out mark to every rank (every rank reports the failure and the
    time-out).  Both ways every rank agrees, and the next step is right."""
    monkeypatch.delenv("CXK_NO_FUSED_TREE", raising=False)
    monkeypatch.delenv("CXK_NO_FUSED_SHARD", raising=False)
    prob, W = _program("c4", 11)
    ref = _reference("c4")
    o = syn.build(ol.Program, prob, "lmi")
    for i in range(len(prob["cliques"])):
        o.set_W(i, W[i])
    o.assemble()
    Kd = o.kkt_matrix()
    c_weight = 0.6 * 0.7
    eig_ref = o.weighted_slack_eigenvalues(ref[1], c_weight)
    rhs = np.random.default_rng(5).uniform(-1, 1, len(ref[1]))
    solve_ref = np.linalg.solve(Kd, rhs)
    v = world - 1

    def body(rank, allreduce):
        k = _rank_context(prob, "c4", rank, world, allreduce, W)
        out = [_step(k, *STEPS[0])]
        if rank == v:
            k.debug_fused_timeout_at(0, KktContext.DEBUG_FUSED_SHARD_TOP | KktContext.DEBUG_FUSED_STREAM_ORDERED)
        k.kkt_solve_async(*STEPS[1])
        got = k.weighted_slack_eigenvalues(None, c_weight) if between == "eigenvalues" else k.solve_inplace(rhs)
        status = k.factor_status()
        out.append({"status": status, "sync": k.sync(), "timed_out": k.fused_tree_timed_out(),
                    "fused": k.fused_tree(), "got": got})
        out.append(_step(k, *STEPS[2]))
        return out

    res = ThreadRanks(world).run(body)
    status = _agree(res, 1, "status")
    assert _agree(res, 1, "sync") == status
    timed_out = _agree(res, 1, "timed_out")
    fused_after = [r[1]["fused"] for r in res]
    if status == 1:          # redone by the victim before the query went out
        assert not timed_out and fused_after == [r != v for r in range(world)]
        for r in res:
            if between == "eigenvalues":
                assert np.allclose(r[1]["got"], eig_ref, rtol=1e-9, atol=0), (r[1]["got"], eig_ref)
            else:
                err = np.linalg.norm(r[1]["got"] - solve_ref) / np.linalg.norm(solve_ref)
                assert err <= TOL, err
    else:                    # the query carried the mark: every rank redoes its iteration
        assert timed_out and not any(fused_after)
    assert _agree(res, 2, "status") == _agree(res, 2, "sync") == 1
    assert not _agree(res, 2, "timed_out")
    for rank, steps in enumerate(res):
        err = np.linalg.norm(steps[2]["y"] - ref[2]) / np.linalg.norm(ref[2])
        assert err <= TOL, f"rank {rank}: relative error {err:.3e}"
