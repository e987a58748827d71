"""Hermitian matrix inequalities given by their entries (cxk_add_hermitian_coo) and the folded sums of the sparse route
(cxk_set_sparse_fold; kernels_lmi_sparse.hip.h, "The folded sums") on the GPU.

 - With fold = 0 the entry point runs the unfolded kernels on device lists identical to those that cxk_add_hermitian
   reads off the dense real representations under CXK_SPARSE_LMI=1: every output is the same bits.
 - With fold = 1 the folded kernels are compared with the CPU oracle on the densified planes, by the comparisons and bars
   of test_gpu_parity.check_newton_step (Schur blocks 1e-13, direction 1e-10, updates 1e-11), one case per instance and
   per number of lanes a pair is shared by.  The extreme Ritz values are not compared (lanczos_tol = inf), as in
   tests/test_gpu_lmi_entries.py: the slack is sparse, and the stage that forms them is not touched here.
"""
import numpy as np
import pytest

import lmi_hermitian_entries_cases as hc
import oracle_lib as ol
from conex_amd import KktContext
from conex_amd import synthetic as syn
from test_gpu_parity import check_newton_step, rel

pytestmark = pytest.mark.gpu


def problem(n, d, m, specs, seed=11):
    """len(specs) constraints of order n over d planes in m variables each on a chain of cliques, member k from
    make_case(**specs[k])."""
    K = len(specs)
    cliques, num_vars = syn.chain_cliques(K, m, 1 if m > 1 else 0)
    cases = [hc.make_case(n, d, m, seed=hc.SEED + 77 * k, **spec) for k, spec in enumerate(specs)]
    b = np.random.default_rng(seed + n + m).uniform(-1, 1, num_vars)
    return dict(cases=cases, cliques=cliques, num_vars=num_vars, b=b, n=n, d=d, m=m, K=K)


def from_entries(prob, fold=None, affine=None):
    k = KktContext(prob["num_vars"], device=0)
    if fold is not None:
        k.set_sparse_fold(fold)
    if affine is not None:
        k.set_sparse_affine(affine)
    for i, (c, cl) in enumerate(zip(prob["cases"], prob["cliques"])):
        assert k.add_hermitian_coo(prob["n"], prob["d"], c["ptr"], c["row"], c["col"], c["val"], cl) == i
    k.initialize()
    return k


def from_planes(cls, prob, fold=None, **kw):
    p = cls(prob["num_vars"], **kw)
    if fold is not None:
        p.set_sparse_fold(fold)
    for i, (c, cl) in enumerate(zip(prob["cases"], prob["cliques"])):
        assert p.add_hermitian(c["A"], c["C"], cl) == i
    p.initialize()
    return p


def set_points(prob, *ctxs):
    W = syn.hermitian_scaling_points(prob["K"], prob["n"], prob["d"])  # W != I
    for p in ctxs:
        for i in range(prob["K"]):
            p.set_W(i, W[i])


def assembled(k, K):
    k.assemble()
    out = []
    for i in range(K):
        G, AW, AQc, sc = k.constraint_schur(i)
        out += [np.tril(G), AW, AQc, sc]
    return out


def lanes_per_pair(prob, fold=True):
    """UploadSparseLmi's rule on the group's lists: the average number of terms of a pair, top x full when folded."""
    m1, d = prob["m"] + 1, prob["d"]
    counts = [[len(hc.embedded_list(c, i)[0]) for i in range(m1)] for c in prob["cases"]]
    cdense = any(c[-1] > 64 for c in counts)
    total = sum(sum(c[:-1] if cdense else c) for c in counts)
    per = total / (len(counts) * m1)
    terms = per * per / (d if fold else 1)
    return 1 if terms <= 8 else 4 if terms <= 64 else 16 if terms <= 1024 else 64


# ------------------------------------------------------------------------------------ fold off: the parent's bits
@pytest.mark.parametrize("n,d,m,spec,name", [
    (4, 2, 1, dict(per=2), "lmi_schur_sparse small"),                     # one block
    (8, 2, 3, dict(per=2, c="full"), "lmi_schur_sparse small dense-C"),
    (36, 2, 3, dict(per=3), "lmi_schur_sparse hbm dense-C"),              # C = I: 72 nonzeros in the real representation
    (17, 4, 2, dict(per=3), "lmi_schur_sparse hbm dense-C"),
])
def test_fold_off_gives_the_bits_of_the_dense_entry_point(monkeypatch, n, d, m, spec, name):
    monkeypatch.setenv("CXK_SPARSE_LMI", "1")
    prob = problem(n, d, m, [spec, spec])                                 # two members with differing lists
    a, p = from_entries(prob, 0), from_planes(KktContext, prob, device=0)
    assert a.count_sparse_lmi() == p.count_sparse_lmi() == 2 and a.count_sparse_fold() == p.count_sparse_fold() == 0
    assert a.lmi_kernels(0) == p.lmi_kernels(0) and a.lmi_kernels(0)["schur"] == name
    set_points(prob, a, p)
    for x, y in zip(assembled(a, 2), assembled(p, 2)):
        assert np.array_equal(x, y)
    y = np.random.default_rng(3).uniform(-0.05, 0.05, a.N)
    assert np.array_equal(a.weighted_slack_eigenvalues(y, 0.56), p.weighted_slack_eigenvalues(y, 0.56))
    ia, ip = a.prepare_step(y, 0.56, 1.0), p.prepare_step(y, 0.56, 1.0)
    assert np.array_equal(ia, ip)
    step = min(1.0, 2.0 / (ia[1] * ia[1]))
    a.take_step(step), p.take_step(step)
    for i in range(2):
        assert np.array_equal(a.get_W(i), p.get_W(i))
    for x, y in zip(assembled(a, 2), assembled(p, 2)):                    # and from the updated W
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------ the folded kernels against the oracle
FOLDED_CASES = [
    # n, d, m, members, sparse_affine, lanes per pair, instance
    (4, 2, 5, [dict(per=(1, 1, 1, 1, 2), off_planes=(1,))] * 2, None, 1, "small"),
    (8, 2, 3, [dict(per=2, c="full")] * 2, None, 4, "small dense-C"),
    (3, 4, 3, [dict(per=1)] * 2, None, 4, "small"),                       # about 6 real entries a matrix
    (6, 4, 3, [dict(per=2, off_planes=(1, 2))] * 2, None, 16, "small"),   # about 20
    (36, 2, 3, [dict(per=3), dict(per=2)], None, 4, "hbm dense-C"),
    (36, 2, 3, [dict(per=3), dict(per=2)], 1, 4, "hbm sparse-C"),
    (17, 4, 2, [dict(per=3)], 1, 16, "hbm sparse-C"),
    (36, 2, 3, [dict(full_a=True)], None, 64, "hbm dense-C"),             # 15 336 real entries: not staged in LDS
]


@pytest.mark.parametrize("n,d,m,specs,affine,lpp,instance", FOLDED_CASES)
def test_folded_newton_step(n, d, m, specs, affine, lpp, instance):
    prob = problem(n, d, m, specs)
    assert lanes_per_pair(prob) == lpp
    if specs[0].get("full_a"):
        assert sum(len(hc.embedded_list(prob["cases"][0], i)[0]) for i in range(m)) > 13600
    k, o = from_entries(prob, None, affine), from_planes(ol.Program, prob)
    assert k.count_sparse_fold() == k.count_sparse_lmi() == len(specs)
    assert k.count_sparse_affine() == (len(specs) if affine else 0)
    assert all(k.lmi_kernels(i)["schur"] == f"lmi_schur_sparse {instance} folded" for i in range(len(specs)))
    set_points(prob, k, o)
    check_newton_step(o, k, prob["b"], lanczos_tol=np.inf)


ASSEMBLY_CASES = [
    # n, d, m, member, sparse_affine, instance, the all-zero matrix
    (36, 2, 3, dict(per=3, c_diag=32), None, "hbm", None),                # 64 nonzeros of L(C): C rides in the pair sums
    (5, 2, 3, dict(per=2, empty_a=1), None, "small", 1),
    (36, 2, 3, dict(per=3, empty_a=0), None, "hbm dense-C", 0),
    (36, 2, 3, dict(per=3, empty_a=2), 1, "hbm sparse-C", 2),
    (9, 2, 4, dict(per=3, off_planes=(1,)), None, "small", None),         # purely imaginary off the diagonal
    (36, 2, 3, dict(per=3, off_planes=(1,)), None, "hbm dense-C", None),
    (7, 4, 3, dict(per=3, off_planes=(3,)), None, "small", None),         # the last plane alone
    (17, 4, 3, dict(per=3, off_planes=(3,)), 1, "hbm sparse-C", None),
    (9, 2, 4, dict(per=2, diag_only=True), None, "small", None),
    (17, 4, 3, dict(per=2, diag_only=True), None, "hbm dense-C", None),
]


@pytest.mark.parametrize("n,d,m,spec,affine,instance,empty", ASSEMBLY_CASES)
def test_folded_assembly(n, d, m, spec, affine, instance, empty):
    """Cases whose Schur matrix is singular or whose C is not definite: the assembled blocks alone."""
    prob = problem(n, d, m, [spec])
    k, o = from_entries(prob, None, affine), from_planes(ol.Program, prob)
    assert k.count_sparse_fold() == 1 and k.lmi_kernels(0)["schur"] == f"lmi_schur_sparse {instance} folded"
    set_points(prob, k, o)
    o.assemble()
    Gk, AWk, AQk, sck = assembled(k, 1)
    Go, AWo, AQo, sco = o.constraint_schur(0)
    print(f"G {rel(Gk, np.tril(Go)):.3g}, AW {rel(AWk, AWo):.3g}, AQc {rel(AQk, AQo):.3g}, scalars {rel(sck, sco):.3g}")
    assert rel(Gk, np.tril(Go)) <= 1e-13 and rel(AWk, AWo) <= 1e-13 and rel(AQk, AQo) <= 1e-13 and rel(sck, sco) <= 1e-13
    if empty is not None:
        assert AQk[empty] == 0.0 and AWk[empty] == 0.0 and not Gk[empty].any() and not Gk[:, empty].any()


# ------------------------------------------------------------------------------------ modes, groups, reproducibility
MODES_PROBLEM = (36, 2, 3, [dict(per=3), dict(per=2), dict(per=4)])


def test_the_two_modes_agree():
    """The bar of test_gpu_lmi_entries.test_the_two_modes_agree: the solutions of one KKT solve within 1e-12."""
    prob = problem(*MODES_PROBLEM)
    ys = []
    for fold in (0, 1):
        k = from_entries(prob, fold)
        assert k.count_sparse_fold() == (3 if fold else 0)
        set_points(prob, k)
        k.set_cost(prob["b"])
        k.kkt_solve_async(0.7, 0.9, 0.8)
        assert k.sync()
        ys.append(k.get_y())
    assert rel(ys[1], ys[0]) <= 1e-12


@pytest.mark.parametrize("shape", [MODES_PROBLEM, (6, 4, 3, [dict(per=2), dict(per=3)])])
def test_two_runs_give_the_same_bits(shape):
    prob = problem(*shape)
    runs = []
    for _ in range(2):
        k = from_entries(prob)
        assert k.count_sparse_fold() == prob["K"]
        set_points(prob, k)
        first = assembled(k, prob["K"])
        again = assembled(k, prob["K"])                   # the same context a second time
        assert all(np.array_equal(x, y) for x, y in zip(first, again))
        k.set_cost(prob["b"])
        k.kkt_solve_async(0.7, 0.9, 0.8)
        assert k.sync()
        runs.append(first + [k.get_y().copy()])
    assert all(np.array_equal(x, y) for x, y in zip(*runs))


def mixed_context(prob):
    """Constraint 0 through add_hermitian, constraint 1 through add_hermitian_coo, no call."""
    k, o = KktContext(prob["num_vars"], device=0), ol.Program(prob["num_vars"])
    c0, c1 = prob["cases"]
    assert k.add_hermitian(c0["A"], c0["C"], prob["cliques"][0]) == 0
    assert k.add_hermitian_coo(prob["n"], prob["d"], c1["ptr"], c1["row"], c1["col"], c1["val"], prob["cliques"][1]) == 1
    for i, c in enumerate(prob["cases"]):
        assert o.add_hermitian(c["A"], c["C"], prob["cliques"][i]) == i
    k.initialize(), o.initialize()
    return k, o


def test_each_entry_point_keeps_its_default_and_the_two_do_not_share_a_group(monkeypatch):
    monkeypatch.setenv("CXK_SPARSE_LMI", "1")
    prob = problem(36, 2, 3, [dict(per=3), dict(per=3)])
    k, o = mixed_context(prob)
    assert (k.count_sparse_lmi(), k.count_sparse_fold(), k.count_sparse_affine()) == (2, 1, 0)
    names = [k.lmi_kernels(i) for i in range(2)]
    assert names[0]["schur"] == "lmi_schur_sparse hbm dense-C"            # today's name and kernels
    assert names[1]["schur"] == "lmi_schur_sparse hbm dense-C folded"     # (one kernel a group: two groups)
    assert {s: v for s, v in names[0].items() if s != "schur"} == {s: v for s, v in names[1].items() if s != "schur"}
    alone = from_planes(KktContext, dict(prob, cases=prob["cases"][:1], cliques=prob["cliques"][:1], K=1), device=0)
    assert alone.lmi_kernels(0) == names[0]
    set_points(prob, k, o)
    check_newton_step(o, k, prob["b"], lanczos_tol=np.inf)


def test_the_environment_switch_folds_a_constraint_added_with_its_planes(monkeypatch):
    monkeypatch.setenv("CXK_SPARSE_LMI", "1")
    monkeypatch.setenv("CXK_SPARSE_FOLD", "1")
    prob = problem(36, 2, 3, [dict(per=3), dict(per=3)])
    k, o = mixed_context(prob)
    assert (k.count_sparse_lmi(), k.count_sparse_fold()) == (2, 2)
    assert all(k.lmi_kernels(i)["schur"] == "lmi_schur_sparse hbm dense-C folded" for i in range(2))
    set_points(prob, k, o)
    check_newton_step(o, k, prob["b"], lanczos_tol=np.inf)
    monkeypatch.setenv("CXK_SPARSE_FOLD", "0")                            # ... and 0 unfolds the one given by entries
    k0 = from_entries(prob)
    assert k0.count_sparse_fold() == 0 and k0.lmi_kernels(1)["schur"] == "lmi_schur_sparse hbm dense-C"


@pytest.mark.parametrize("n,m,c", [(9, 3, "identity"), (70, 3, "identity"), (9, 2, "full")])
def test_over_the_reals_nothing_folds_and_the_sums_are_those_of_add_lmi_coo(n, m, c):
    """d = 1: herm_d = 1 keeps the Hermitian step rules, so the assembly is what is compared with add_lmi_coo's."""
    prob = problem(n, 1, m, [dict(per=3, c=c), dict(per=2, c=c)])
    k = from_entries(prob, 1)                                             # even when asked for
    r = KktContext(prob["num_vars"], device=0)
    r.set_sparse_affine(0)                                                # (this entry point's default for the affine term)
    for i, (case, cl) in enumerate(zip(prob["cases"], prob["cliques"])):
        assert r.add_lmi_coo(n, case["ptr"], case["row"], case["col"], case["val"][:, 0], cl) == i
    r.initialize()
    assert k.count_sparse_fold() == 0 and k.count_sparse_lmi() == 2
    assert k.lmi_kernels(0)["schur"] == r.lmi_kernels(0)["schur"] and not k.lmi_kernels(0)["schur"].endswith("folded")
    W = syn.scaling_points(2, n)
    for i in range(2):
        k.set_W(i, W[i][None]), r.set_W(i, W[i])
    for x, y in zip(assembled(k, 2), assembled(r, 2)):
        assert np.array_equal(x, y)
