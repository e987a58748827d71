"""KktContext.solve_block (cxk_solve_block / cxk_solve_block_device): K^-1 applied to a block of right-hand sides
with the stored factor, behind every route that leaves a factor.

Reference and bound: column j of the block solve against the oracle's solve_inplace of column j on the same
scaling points and the same assembled system, rel <= TOL_DIRECTION (test_gpu_parity.py's bound for solve_inplace
on an arbitrary host vector, imported); and against the context's own solve_inplace of that column under the
same bound.  All tests need a real MI355X.
"""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
from conex_amd import KktContext
from conex_amd import synthetic as syn
from conex_amd.kkt import KktError
from test_gpu_parity import TOL_DIRECTION, rel

pytestmark = pytest.mark.gpu

CHUNK = None  # cxk_solve_block_chunk_width(), read once


def chunk_width():
    global CHUNK
    if CHUNK is None:
        from conex_amd.kkt import load_library
        CHUNK = int(load_library().cxk_solve_block_chunk_width())
    return CHUNK


def build_with_env(env, make):
    """The switches are read once, when a context is initialized: set them around the build only."""
    saved = {v: os.environ.get(v) for v in env}
    os.environ.update(env)
    try:
        return make()
    finally:
        for v, old in saved.items():
            if old is None:
                os.environ.pop(v, None)
            else:
                os.environ[v] = old


def factored(o, k, W=None):
    if W is not None:
        for i in range(len(W)):
            o.set_W(i, W[i])
            k.set_W(i, W[i])
    o.assemble()
    k.assemble()
    assert o.factor() == 1 and k.factor() == 1
    return o, k


# ------------------------------------------------------------------ a small LMI tree shared by several tests
_SMALL = {}


def small_tree():
    """lmi_problem(K=9, n=6, m=6): oracle, factored context, 2 * chunk + 1 right-hand sides and the oracle's
    solutions, computed once and never changed."""
    if not _SMALL:
        prob = syn.lmi_problem(K=9, n=6, m=6, branching=2, overlap=2, seed=109)
        W = syn.scaling_points(9, 6, seed=16)
        o = syn.build(ol.Program, prob, "lmi")
        k = syn.build(KktContext, prob, "lmi", device=0)
        factored(o, k, W)
        B = np.random.default_rng(1).uniform(-1, 1, (k.N, 2 * chunk_width() + 1))
        ref = np.stack([o.solve_inplace(B[:, j]) for j in range(B.shape[1])], axis=1)
        B.setflags(write=False)
        ref.setflags(write=False)
        _SMALL.update(prob=prob, W=W, o=o, k=k, B=B, ref=ref)
    return _SMALL


def column_counts():
    w = 32  # kSbW; checked against the library in the test
    return sorted({1, 2, 3, 15, 16, 17, w - 1, w, w + 1, 2 * w + 1})


# ------------------------------------------------------------------ 1: column counts and leading dimensions
@pytest.mark.parametrize("nrhs", column_counts())
def test_column_counts_and_leading_dimension(nrhs):
    s = small_tree()
    w = chunk_width()
    assert {w - 1, w, w + 1, 2 * w + 1} <= set(column_counts())
    k, N = s["k"], s["k"].N
    B = s["B"][:, :nrhs]
    X = k.solve_block(B)                      # ld = N
    for j in range(nrhs):
        assert rel(X[:, j], s["ref"][:, j]) <= TOL_DIRECTION
        if j in (0, nrhs - 1):
            assert rel(X[:, j], k.solve_inplace(B[:, j])) <= TOL_DIRECTION
    # ld = N + 3 through the C entry point: the padding rows hold a sentinel and keep it
    sentinel = -7.25e300
    buf = np.full((nrhs, N + 3), sentinel)    # row j of this C-ordered array is column j with ld = N + 3
    buf[:, :N] = B.T
    k._check(k.L.cxk_solve_block(k.h, buf.ctypes.data_as(C.POINTER(C.c_double)), N + 3, nrhs), "cxk_solve_block")
    assert np.array_equal(buf[:, N:], np.full((nrhs, 3), sentinel))
    assert np.array_equal(buf[:, :N].T, X)    # the same solve: the same bits


def test_one_dimensional_input_is_one_column():
    s = small_tree()
    x = s["k"].solve_block(s["B"][:, 0])
    assert x.shape == (s["k"].N,)
    assert rel(x, s["ref"][:, 0]) <= TOL_DIRECTION
    # any memory order is taken
    Bc = np.ascontiguousarray(s["B"][:, :5])
    Bf = np.asfortranarray(s["B"][:, :5])
    assert np.array_equal(s["k"].solve_block(Bc), s["k"].solve_block(Bf))


# ------------------------------------------------------------------ 2: factor routes
def _lmi_pair(K, n, m, b_, ov, seed, wseed, env=None):
    prob = syn.lmi_problem(K=K, n=n, m=m, branching=b_, overlap=ov, seed=seed)
    W = syn.scaling_points(K, n, seed=wseed)
    o = syn.build(ol.Program, prob, "lmi")
    k = build_with_env(env or {}, lambda: syn.build(KktContext, prob, "lmi", device=0))
    return factored(o, k, W)


def _route_small_tree_fused():
    o, k = _lmi_pair(9, 6, 6, 2, 2, 109, 16)
    assert k.fused_tree() == 1
    return o, k


def _route_small_tree_levels():
    o, k = _lmi_pair(9, 6, 6, 2, 2, 109, 16, {"CXK_NO_FUSED_TREE": "1"})
    assert k.fused_tree() == 0
    return o, k


def _route_mixed():
    prob = syn.mixed_problem(K=46, herm_every=(4, 7), branching=4, overlap=3)
    W = syn.mixed_scaling_points(prob, seed=32)
    o = syn.build(ol.Program, prob, "mixed")
    k = syn.build(KktContext, prob, "mixed", device=0)
    return factored(o, k, W)


def _route_chain(segments):
    def make():
        prob = syn.soc_problem(K=40, tree=0)
        W = syn.soc_scaling_points(40, 10)
        o = syn.build(ol.Program, prob, "soc")
        k = build_with_env({"CXK_CHAIN_SEGMENTS": segments}, lambda: syn.build(KktContext, prob, "soc", device=0))
        assert (k.chain_segments() != 0) == (segments != "0")
        return factored(o, k, W)
    return make


def _route_wide_root(num_vars, rows):
    def make():
        prob = syn.lp_problem(rows=rows, num_vars=num_vars, seed=num_vars)
        o = syn.build(ol.Program, prob, "lp")
        k = syn.build(KktContext, prob, "lp", device=0)
        assert max(k.supernode_sizes()) == num_vars
        return factored(o, k)
    return make


def _route_dense_top():
    o, k = _lmi_pair(1, 52, 40, 2, 1, 340, 55)
    assert k.dense_top_columns() > 0
    return o, k


def _route_lqr(N):
    def make():
        from test_oracle_kat import build_lqr_problem
        o = build_lqr_problem(ol.Program, N)
        k = build_lqr_problem(KktContext, N, device=0)
        assert k.N == (N + 1) * 3 + 2 * (N + 1)
        factored(o, k)
        assert k.factor_regularized() == 0
        return o, k
    return make


def _route_four_cycle():
    cliques = [[0, 1], [1, 2], [0, 3], [2, 3]]   # needs fill-in: the tree has empty supernodes

    def build(cls, **kw):
        rng0 = np.random.default_rng(4)
        p = cls(4, **kw)
        A = rng0.uniform(-1, 1, (2, 3, 3))
        A = 0.5 * (A + np.transpose(A, (0, 2, 1)))
        p.add_lmi(A, np.eye(3), cliques[0])
        p.add_soc(rng0.uniform(-1, 1, (4, 2)), np.array([1.0, 0, 0, 0]), cliques[1])
        p.add_linear(rng0.uniform(-1, 1, (5, 2)), np.abs(rng0.uniform(0.5, 1, 5)), cliques[2])
        p.add_static(np.array([[2.0, 0.3], [0.3, 1.0]]), cliques[3])
        p.initialize()
        return p
    o, k = build(ol.Program), build(KktContext, device=0)
    assert min(k.supernode_sizes()) == 0
    return factored(o, k)


ROUTES = {
    "small-tree-fused": _route_small_tree_fused,
    "small-tree-level-kernels": _route_small_tree_levels,
    "mixed-shapes": _route_mixed,
    "chain-segmented": _route_chain("4"),
    "chain-reference-order": _route_chain("0"),
    "root-wider-than-64": _route_wide_root(70, 100),
    "root-wider-than-128": _route_wide_root(130, 170),
    "dense-top": _route_dense_top,
    "ldlt-lqr-2": _route_lqr(2),
    "ldlt-lqr-40": _route_lqr(40),
    "four-cycle-empty-supernodes": _route_four_cycle,
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_factor_routes(route):
    o, k = ROUTES[route]()
    w = chunk_width()
    B = np.random.default_rng(5).uniform(-1, 1, (k.N, w + 2))   # two chunks, the second ragged
    X = k.solve_block(B)
    cols = range(B.shape[1]) if k.N <= 400 else (0, 1, w - 1, w, w + 1)
    for j in cols:
        want = o.solve_inplace(B[:, j])
        assert rel(X[:, j], want) <= TOL_DIRECTION, (route, j, rel(X[:, j], want))
        own = k.solve_inplace(B[:, j])
        assert rel(X[:, j], own) <= TOL_DIRECTION, (route, j, rel(X[:, j], own))
    assert np.array_equal(k.solve_block(B[:, :3]), X[:, :3])


# ------------------------------------------------------------------ 3: column independence, reproducibility
def test_columns_are_independent_and_runs_are_bit_reproducible():
    s = small_tree()
    k, N = s["k"], s["k"].N
    w = chunk_width()
    b = s["B"][:, :1]
    J = np.random.default_rng(9).uniform(-1, 1, (N, w + 1))     # neighbours in the same chunk and in the next
    runs = [k.solve_block(np.hstack([b, Jx])) for Jx in (J, np.zeros_like(J), np.full_like(J, np.nan))]
    assert np.array_equal(runs[0][:, 0], runs[1][:, 0]) and np.array_equal(runs[0][:, 0], runs[2][:, 0])
    assert np.all(np.isfinite(runs[2][:, 0])) and np.all(np.isnan(runs[2][:, 1:]))
    # the NaN stays in its column
    M = np.hstack([b, J])
    M[3, 2] = np.nan
    Xn = k.solve_block(M)
    assert np.all(np.isnan(Xn[:, 2]))
    keep = [j for j in range(M.shape[1]) if j != 2]
    assert np.array_equal(Xn[:, keep], runs[0][:, keep])
    assert np.array_equal(k.solve_block(np.hstack([b, J])), runs[0])


# ------------------------------------------------------------------ 4: the rest of the context's state
def test_state_is_left_alone():
    s = small_tree()
    k = s["k"]
    k.set_y(np.arange(1.0, k.N + 1))
    before = (k.get_y(), [k.get_W(i) for i in range(k.K)], k.slab())
    k.solve_block(s["B"][:, :chunk_width() + 1])
    after = (k.get_y(), [k.get_W(i) for i in range(k.K)], k.slab())
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[2], after[2])
    assert all(np.array_equal(a, b) for a, b in zip(before[1], after[1]))


def test_block_solve_between_the_triple_launch_and_the_direction():
    """assemble -> factor_solve_triple_async -> [solve_block] -> select_mu_async -> newton_direction_device_mu: the
    direction is the one obtained without the block solve in between, bit for bit."""
    prob = syn.lmi_problem(K=40, n=20, m=20, branching=4, overlap=5, seed=5)
    W = syn.scaling_points(40, 20, seed=10)
    bs, cs = 0.9, 0.8
    ys = []
    for with_block in (False, True):
        k = syn.build(KktContext, prob, "lmi", device=0)
        for i in range(k.K):
            k.set_W(i, W[i])
        k.set_cost(prob["b"])
        k.assemble()
        assert k.L.cxk_triple_supported(k.h) == 1
        k._check(k.L.cxk_factor_solve_triple_async(k.h, bs, cs), "cxk_factor_solve_triple_async")
        if with_block:
            B = np.random.default_rng(3).uniform(-1, 1, (k.N, 5))
            X = k.solve_block(B)
            assert np.all(np.isfinite(X))
        k._check(k.L.cxk_select_mu_async(k.h, cs, 1.0, 800, 0.3, 0.75, 0.75), "cxk_select_mu_async")
        k._check(k.L.cxk_newton_direction_device_mu(k.h, bs, cs), "cxk_newton_direction_device_mu")
        ys.append(k.get_y())
        if with_block:   # and the block solve was a solve with that factor
            assert rel(X[:, 0], k.solve_inplace(B[:, 0])) <= TOL_DIRECTION
    assert np.all(np.isfinite(ys[0])) and np.array_equal(ys[0], ys[1])


# ------------------------------------------------------------------ 5: refusals
def _tiny():
    prob = syn.lmi_problem(K=5, n=4, m=4, branching=2, overlap=2, seed=3)
    return prob, syn.build(KktContext, prob, "lmi", device=0)


def _raw(k, B, ld, nrhs):
    k._check(k.L.cxk_solve_block(k.h, B.ctypes.data_as(C.POINTER(C.c_double)), ld, nrhs), "cxk_solve_block")


def test_refusals_name_their_cause():
    prob, k = _tiny()
    B = np.ones((k.N, 2))
    with pytest.raises(KktError, match="no factorization yet"):
        k.solve_block(B)
    for i in range(k.K):
        k.set_W(i, np.zeros((4, 4)))     # singular scaling point: zero Schur complement
    k.assemble()
    assert k.factor() == 0
    with pytest.raises(KktError, match="latest factorization failed"):
        k.solve_block(B)
    W = syn.scaling_points(5, 4, seed=2)
    for i in range(k.K):
        k.set_W(i, W[i])
    k.assemble()
    assert k.factor() == 1
    X = k.solve_block(B)
    F = np.asfortranarray(B)
    with pytest.raises(KktError, match="nrhs must be at least 1"):
        _raw(k, F, k.N, 0)
    with pytest.raises(KktError, match="leading dimension"):
        _raw(k, F, k.N - 1, 2)
    with pytest.raises(KktError, match="null pointer"):
        k._check(k.L.cxk_solve_block(k.h, None, k.N, 2), "cxk_solve_block")
    k.set_refinement(1)
    with pytest.raises(KktError, match="iterative refinement"):
        k.solve_block(B)
    k.set_refinement(0)
    assert np.array_equal(k.solve_block(B), X)   # nothing of the refused calls stuck


def test_qr_mode_is_refused():
    prob, k = _tiny()
    k.set_solver_mode(2)
    k.assemble()
    assert k.factor() == 1
    with pytest.raises(KktError, match="QR solver mode"):
        k.solve_block(np.ones((k.N, 2)))


# ------------------------------------------------------------------ 6: torch tensors on the device
TORCH_CHILD = r"""
import sys
import numpy as np
import torch
torch.cuda.init()                 # torch's GPU state first, the library's second: the order bench.py uses
sys.path[:0] = [%(root)r, %(tests)r]
from conex_amd import KktContext, synthetic as syn
prob = syn.lmi_problem(K=9, n=6, m=6, branching=2, overlap=2, seed=109)
W = syn.scaling_points(9, 6, seed=16)
k = syn.build(KktContext, prob, "lmi", device=0)
for i in range(k.K):
    k.set_W(i, W[i])
k.assemble()
assert k.factor() == 1
w = k.L.cxk_solve_block_chunk_width()
B = np.random.default_rng(1).uniform(-1, 1, (k.N, w + 3))
X = k.solve_block(B)
t = torch.from_numpy(B).to("cuda:0").T.contiguous().T      # column-major storage
assert t.stride(0) == 1
out = k.solve_block(t)
assert out is t
assert np.array_equal(t.cpu().numpy(), X), "torch path and numpy path differ"
wide = torch.zeros((w + 3, k.N + 5), dtype=torch.float64, device="cuda:0").T[:k.N]   # ld = N + 5
wide.copy_(torch.from_numpy(B))
assert np.array_equal(k.solve_block(wide).cpu().numpy(), X)
for bad, what in ((torch.from_numpy(B).to("cuda:0"), "column-major"), (t.float(), "float64"),
                  (torch.from_numpy(B).T.contiguous().T, "on the GPU"), (t[:-1], "expected shape")):
    try:
        k.solve_block(bad)
    except ValueError as e:
        assert what in str(e), (what, str(e))
    else:
        raise AssertionError("accepted: " + what)
print("TORCH-OK")
"""


def test_torch_tensor_is_solved_in_place():
    """A column-major ROCm tensor is solved in place, bit for bit the numpy path; anything else is a ValueError.
    In a child process: torch does not find the GPU in a process where the library has initialised HIP before it
    ("No HIP GPUs are available"), so torch's GPU state has to come first, and this suite's process is past that."""
    import subprocess
    import sys
    tests = os.path.dirname(os.path.abspath(__file__))
    code = TORCH_CHILD % {"root": os.path.dirname(tests), "tests": tests}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "TORCH-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
