"""Matrix inequalities given by their entries (cxk_add_lmi_coo) and the affine term evaluated from its nonzeros
(cxk_set_sparse_affine; kernels_lmi_sparse.hip.h: lmi_affine_wc / _x / _scalars) on the GPU.

 - With sparse_affine = 0 the entry point runs today's kernels on device lists identical to those that cxk_add_lmi
   reads off the dense matrices under CXK_SPARSE_LMI=1: every output is the same bits.
 - With sparse_affine = 1 the new kernels are compared with the CPU oracle on the densified data, by the comparisons and
   bars of tests/test_gpu_sparse.py (test_gpu_parity.check_newton_step: Schur blocks 1e-13, direction 1e-10, updates
   1e-11).  The extreme Ritz values are not compared (lanczos_tol = inf), as in test_sparse_large_order beyond order 70:
   the slack is sparse - k I, on which the reference's unreorthogonalised Lanczos run breaks down early, and the stage
   that forms them is not touched here; slack traces, norms and the updated W are compared.
"""
import numpy as np
import pytest

import lmi_entries_cases as ec
import oracle_lib as ol
from conex_amd import KktContext
from conex_amd import synthetic as syn
from test_gpu_parity import check_newton_step, rel

pytestmark = pytest.mark.gpu

NEW_NAME = "lmi_schur_sparse hbm sparse-C"


def problem(n, m, specs, seed=11):
    """len(specs) constraints of order n over m variables each on a chain of cliques, member k from make_case(**specs[k])."""
    K = len(specs)
    cliques, num_vars = syn.chain_cliques(K, m, 1 if m > 1 else 0)
    cases = [ec.make_case(n, m, seed=ec.SEED + 77 * k, **spec) for k, spec in enumerate(specs)]
    b = np.random.default_rng(seed + n + m).uniform(-1, 1, num_vars)
    return dict(cases=cases, cliques=cliques, num_vars=num_vars, b=b, n=n, m=m, K=K)


def from_entries(prob, mode):
    k = KktContext(prob["num_vars"], device=0)
    if mode is not None:
        k.set_sparse_affine(mode)
    for i, (c, cl) in enumerate(zip(prob["cases"], prob["cliques"])):
        assert k.add_lmi_coo(prob["n"], c["ptr"], c["row"], c["col"], c["val"], cl) == i
    k.initialize()
    return k


def from_matrices(cls, prob, mode=None, **kw):
    p = cls(prob["num_vars"], **kw)
    if mode is not None:
        p.set_sparse_affine(mode)
    for i, (c, cl) in enumerate(zip(prob["cases"], prob["cliques"])):
        assert p.add_lmi(c["A"], c["C"], cl) == i
    p.initialize()
    return p


def set_points(prob, *ctxs, scale=0.1):
    W = syn.scaling_points(prob["K"], prob["n"], scale=scale)
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


# ------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("n,m,nnz", [(9, 1, (40, 33)), (9, 3, (65, 65)), (9, 3, (40, 65)), (64, 3, (65, 120)), (64, 1, (300, 300)),
                                     (65, 3, (65, 64)), (65, 1, (200, 90))])
def test_mode_zero_gives_the_bits_of_the_dense_entry_point(monkeypatch, n, m, nnz):
    """Two members with differing lists; C rides in the pair sums (<= 64 nonzeros) or takes the dense route (LDS at order
    9, the two GEMMs from order 64 on)."""
    monkeypatch.setenv("CXK_SPARSE_LMI", "1")
    prob = problem(n, m, [dict(nnz_c=z) for z in nnz])
    a, d = from_entries(prob, 0), from_matrices(KktContext, prob, device=0)
    assert a.count_sparse_lmi() == d.count_sparse_lmi() == 2 and a.count_sparse_affine() == d.count_sparse_affine() == 0
    assert a.lmi_kernels(0) == d.lmi_kernels(0)
    set_points(prob, a, d)
    for x, y in zip(assembled(a, 2), assembled(d, 2)):
        assert np.array_equal(x, y)
    y = np.random.default_rng(3).uniform(-0.05, 0.05, a.N)
    assert np.array_equal(a.weighted_slack_eigenvalues(y, 0.56), d.weighted_slack_eigenvalues(y, 0.56))
    ia, id_ = a.prepare_step(y, 0.56, 1.0), d.prepare_step(y, 0.56, 1.0)
    assert np.array_equal(ia, id_)
    step = min(1.0, 2.0 / (ia[1] * ia[1]))
    a.take_step(step), d.take_step(step)
    for i in range(2):
        assert np.array_equal(a.get_W(i), d.get_W(i))
    for x, y in zip(assembled(a, 2), assembled(d, 2)):  # and from the updated W
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------ the new kernels against the oracle
ORACLE_CASES = [
    # n (64: the first order beyond LDS), m, members
    (64, 1, [dict(nnz_c=65)]),
    (64, 3, [dict(nnz_c=65), dict(nnz_c=120), dict(nnz_c=301)]),          # a group of three, differing lists
    (65, 7, [dict(nnz_c=65, diag_only=True)]),                            # a diagonal-only C (65 of the 65 possible)
    (65, 3, [dict(nnz_c=101, empty_index=5)]),                            # an empty row and column of C
    (130, 7, [dict(nnz_c=400, empty_index=0), dict(nnz_c=65), dict(nnz_c=130, diag_only=True)]),
    (130, 1, [dict(nnz_c=65)]),
]


@pytest.mark.parametrize("n,m,specs", ORACLE_CASES)
def test_sparse_affine_newton_step(n, m, specs):
    prob = problem(n, m, specs)
    k, o = from_entries(prob, 1), from_matrices(ol.Program, prob)
    assert k.count_sparse_affine() == k.count_sparse_lmi() == len(specs)
    set_points(prob, k, o)                                                # W != I
    check_newton_step(o, k, prob["b"], lanczos_tol=np.inf)


@pytest.mark.parametrize("n,m,specs", [(65, 3, [dict(nnz_c=77, empty_a=1)]),
                                       (130, 7, [dict(nnz_c=65, empty_a=0), dict(nnz_c=200, empty_a=6, empty_index=129),
                                                 dict(nnz_c=66, diag_only=True, empty_a=3)])])
def test_sparse_affine_assembly_with_an_empty_matrix(n, m, specs):
    """An all-zero A_i: its row of G, AW and AQc are zero and the Schur matrix is singular by construction, so only the
    assembled blocks are compared."""
    prob = problem(n, m, specs)
    k, o = from_entries(prob, 1), from_matrices(ol.Program, prob)
    assert k.count_sparse_affine() == len(specs)
    set_points(prob, k, o)
    o.assemble()
    got = assembled(k, len(specs))
    for i, spec in enumerate(specs):
        Go, AWo, AQo, sco = o.constraint_schur(i)
        Gk, AWk, AQk, sck = got[4 * i:4 * i + 4]
        assert rel(Gk, np.tril(Go)) <= 1e-13 and rel(AWk, AWo) <= 1e-13 and rel(AQk, AQo) <= 1e-13 and rel(sck, sco) <= 1e-13
        e = spec["empty_a"]
        assert AQk[e] == 0.0 and AWk[e] == 0.0 and not Gk[e].any() and not Gk[:, e].any()


def test_a_constraint_added_with_its_matrices_runs_the_new_kernels_when_asked(monkeypatch):
    monkeypatch.setenv("CXK_SPARSE_LMI", "1")
    prob = problem(70, 3, [dict(nnz_c=150), dict(nnz_c=90)])
    k, o = from_matrices(KktContext, prob, mode=1, device=0), from_matrices(ol.Program, prob)
    assert k.count_sparse_affine() == 2 and k.lmi_kernels(1)["schur"] == NEW_NAME
    set_points(prob, k, o)
    check_newton_step(o, k, prob["b"], lanczos_tol=np.inf)


def test_a_hermitian_constraint_runs_the_new_kernels_under_the_environment_switch(monkeypatch):
    """Complex Hermitian cones of order 36 (real representation 72, beyond LDS; C = I has 72 nonzeros there), asked for
    through CXK_SPARSE_AFFINE: the real representation goes through the same kernels."""
    monkeypatch.setenv("CXK_SPARSE_LMI", "1")
    monkeypatch.setenv("CXK_SPARSE_AFFINE", "1")
    from test_gpu_parity import make_pair
    K, n, d, m = 2, 36, 2, 6
    prob = syn.sparsify(syn.hermitian_problem(K=K, n=n, d=d, m=m, branching=2, overlap=2), 0.004)
    o, k = make_pair(prob, "herm", syn.hermitian_scaling_points(K, n, d))
    assert k.count_sparse_lmi() == K and k.count_sparse_affine() == K and k.lmi_kernels(0)["schur"] == NEW_NAME
    check_newton_step(o, k, prob["b"], lanczos_tol=np.inf)


# ------------------------------------------------------------------------------------ reproducibility, modes, counts
def test_two_runs_give_the_same_bits():
    prob = problem(130, 7, [dict(nnz_c=400), dict(nnz_c=65), dict(nnz_c=131)])
    runs = []
    for _ in range(2):
        k = from_entries(prob, 1)
        set_points(prob, k)
        first = assembled(k, 3)
        again = assembled(k, 3)                       # the same context a second time
        assert all(np.array_equal(x, y) for x, y in zip(first, again))
        k.set_cost(prob["b"])
        k.kkt_solve_async(0.7, 0.9, 0.8)
        assert k.sync()
        runs.append(first + [k.get_y().copy()])
    assert all(np.array_equal(x, y) for x, y in zip(*runs))


def test_the_two_modes_agree():
    """What test_sparse_and_dense_paths_agree asks of its pair: the solutions of one KKT solve within 1e-12."""
    prob = problem(130, 7, [dict(nnz_c=400), dict(nnz_c=65), dict(nnz_c=131)])
    ys = []
    for mode in (0, 1):
        k = from_entries(prob, mode)
        assert k.count_sparse_affine() == (3 if mode else 0)
        set_points(prob, k)
        k.set_cost(prob["b"])
        k.kkt_solve_async(0.7, 0.9, 0.8)
        assert k.sync()
        ys.append(k.get_y())
    assert rel(ys[1], ys[0]) <= 1e-12


def test_counts_and_the_kernel_name():
    prob = problem(64, 3, [dict(nnz_c=65), dict(nnz_c=120)])
    k = from_entries(prob, 1)
    assert (k.count_sparse_affine(), k.count_sparse_lmi(), k.count_lmi_kernel(4)) == (2, 2, 2)
    assert k.lmi_kernels(0)["schur"] == k.lmi_kernels(1)["schur"] == NEW_NAME
    other = {s: v for s, v in k.lmi_kernels(0).items() if s != "schur"}
    k0 = from_entries(prob, 0)
    assert (k0.count_sparse_affine(), k0.count_sparse_lmi(), k0.count_lmi_kernel(4)) == (0, 2, 2)
    assert k0.lmi_kernels(0)["schur"] == "lmi_schur_sparse hbm dense-C"
    assert {s: v for s, v in k0.lmi_kernels(0).items() if s != "schur"} == other  # no other stage changes its kernel


def test_the_automatic_mode_and_the_groups():
    """Without a call a constraint given by entries asks LmiSparseAffinePays: max-cut-like data moves, a nearly full C
    does not, nor does anything LDS-resident or a C of at most 64 nonzeros; members that differ do not share a group."""
    sparse, full = dict(nnz_c=65), dict(nnz_c=4000)
    prob = problem(64, 3, [sparse, full, sparse])
    k = from_entries(prob, None)
    assert k.count_sparse_lmi() == 3 and k.count_sparse_affine() == 2
    names = [k.lmi_kernels(i)["schur"] for i in range(3)]
    assert names == [NEW_NAME, "lmi_schur_sparse hbm dense-C", NEW_NAME]
    o = from_matrices(ol.Program, prob)
    set_points(prob, k, o)
    check_newton_step(o, k, prob["b"], lanczos_tol=np.inf)
    for n, nnz, name in [(9, 65, "lmi_schur_sparse small dense-C"), (64, 64, "lmi_schur_sparse hbm")]:
        k = from_entries(problem(n, 3, [dict(nnz_c=nnz)]), 1)  # even when asked for: not eligible
        assert k.count_sparse_affine() == 0 and k.count_sparse_lmi() == 1 and k.lmi_kernels(0)["schur"] == name


def test_a_constraint_added_with_its_matrices_keeps_its_kernels_without_a_call(monkeypatch):
    monkeypatch.setenv("CXK_SPARSE_LMI", "1")
    prob = problem(64, 3, [dict(nnz_c=65), dict(nnz_c=120)])
    k = from_matrices(KktContext, prob, device=0)
    assert k.count_sparse_lmi() == 2 and k.count_sparse_affine() == 0
    assert k.lmi_kernels(0)["schur"] == "lmi_schur_sparse hbm dense-C"
