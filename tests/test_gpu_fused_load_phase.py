"""The plan-time load image of the whole-tree launch (tree_fused.h FusedImgLayout): where every lane
finds every entry of its panel, which entries do not exist (they point at a +0.0 behind the Schur arena, padding
pivots at a 1.0), where its row of the right-hand side and of the factor sits, where the published values go.

The image replaces arithmetic on the record, not a floating-point operation: the whole-tree launch must still give
the level kernels' (CXK_NO_FUSED_TREE=1) factor, AW / AQc and scalars BIT FOR BIT and their direction to 1e-13.
The shapes are the smallest at which an image entry can be wrong: fewer columns than the frame (padding pivots and
their unit diagonals), a full frame, the exact-fit pair with further sources and shared rows on two levels, a chain
(a leaf and the root in one launch, every non-leaf with one child), structural fill in the separator rows, leaves in
both frames of a pair -- in every launch form that reads the image: the factor-and-solve, the assemble / factor order
of the interior-point loop, three right-hand sides, the two-launch form."""
import contextlib
import os

import numpy as np
import pytest

from conex_amd import KktContext
from conex_amd import synthetic as syn

pytestmark = pytest.mark.gpu

M = 20  # variables per constraint: a supernode has M - overlap columns and `overlap` separator rows, the root M columns


@contextlib.contextmanager
def environment(**env):
    """The switches are read when a context is built: set (a value) or unset (None) for the block, then put back."""
    before = {name: os.environ.get(name) for name in env}
    try:
        for name, value in env.items():
            if value is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = value
        yield
    finally:
        for name, value in before.items():
            if value is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = value


def build(prob, W, kind="lmi"):
    k = syn.build(KktContext, prob, kind, device=0)
    for i in range(k.K):
        k.set_W(i, W[i])
    k.set_cost(prob["b"])
    return k


def contexts(prob, W, kind="lmi", **env):
    """(whole-tree launch, level kernels) on the same problem and scaling points"""
    with environment(**env):
        with environment(CXK_NO_FUSED_TREE=None):
            fused = build(prob, W, kind)
        with environment(CXK_NO_FUSED_TREE="1"):
            levels = build(prob, W, kind)
    assert fused.fused_tree() and not levels.fused_tree()
    return fused, levels


def snapshot(k):
    AW, AQc, sc = k.residuals()
    if k.chain_segments() != 0:
        # (the library does not hand out a factor stored in the segment-parallel order; the solve on the stored
        # factor at the end of all_launch_forms, compared bit for bit, stands in for it)
        return k.get_y().copy(), AW, AQc, sc
    return k.get_y().copy(), k.slab().copy(), AW, AQc, sc


def assert_factor_bits_direction_close(a, b):
    err = np.linalg.norm(a[0] - b[0]) / np.linalg.norm(b[0])
    print("direction: relative difference %.3e" % err)
    assert err <= 1e-13
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y, equal_nan=True)


def assert_same_bits(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)


# (K, n, branching, overlap, CXK_FUSED_PADDED_FRAMES): 13 + 7 columns, LMIs of order 20 and 12: fewer columns than
# the frame; 16 + 4 in the padded pair: <16, 8> full; 73: the exact-fit pair, three levels; a chain of six
LMI_SHAPES = [(9, 20, 8, 7, None), (9, 12, 8, 7, None), (9, 8, 8, 4, "1"), (73, 20, 8, 5, None), (6, 20, 1, 5, None)]


def lmi_pair(K, n, branching, overlap, padded, seed, **env):
    prob = syn.lmi_problem(K=K, n=n, m=M, branching=branching, overlap=overlap, seed=seed + K + n)
    W = syn.scaling_points(K, n, seed=seed + 1)
    fused, levels = contexts(prob, W, CXK_FUSED_PADDED_FRAMES=padded, **env)
    (na, sa), (nb, sb) = fused.fused_tree_frames()
    if overlap == 7:
        assert na > M - overlap and sa > overlap  # padding pivots, padding separator rows
    elif overlap == 4:
        assert (na, sa) == (16, 8) and M - overlap == na
    else:
        assert ((na, sa), (nb, sb)) == ((16, 5), (20, 0))
    return fused, levels


def all_launch_forms(fused, levels):
    for mu in (0.7, 0.4, 0.9, 0.55, 0.61):  # (five launches: both sets of hand-off slots)
        for k in (fused, levels):
            k.kkt_solve_async(mu, 0.9, 0.8)
            assert k.sync()
        assert_factor_bits_direction_close(snapshot(fused), snapshot(levels))
    for k in (fused, levels):
        k.assemble()
        k.factor_solve_async(-0.9, 0.8, 0.0)
        assert k.sync()
    assert_factor_bits_direction_close(snapshot(fused), snapshot(levels))
    for k in (fused, levels):
        k.solve_rhs(0.3, -0.2, 1.5)
        assert k.sync()
    assert np.array_equal(fused.get_y(), levels.get_y())


@pytest.mark.parametrize("K,n,branching,overlap,padded", LMI_SHAPES)
def test_image_driven_load_equals_level_kernels(K, n, branching, overlap, padded):
    fused, levels = lmi_pair(K, n, branching, overlap, padded, seed=151)
    all_launch_forms(fused, levels)


@pytest.mark.parametrize("K,n,branching,overlap,padded", LMI_SHAPES)
def test_image_driven_load_in_the_two_launch_form(K, n, branching, overlap, padded):
    """CXK_FUSED_SPLIT=1: the way up as a launch of its own (the right-hand side as a column: the other half of every
    publish entry); it sweeps back down as the level kernels do, so the direction is the same bits too."""
    fused, levels = lmi_pair(K, n, branching, overlap, padded, seed=161, CXK_FUSED_SPLIT="1")
    for mu in (0.7, 0.4, 0.9):
        for k in (fused, levels):
            k.kkt_solve_async(mu, 0.9, 0.8)
            assert k.sync()
        assert_same_bits(snapshot(fused), snapshot(levels))


@pytest.mark.parametrize("K,n,branching,overlap,padded", LMI_SHAPES)
def test_image_driven_load_with_three_right_hand_sides(K, n, branching, overlap, padded):
    """The triple launch (cxk_factor_solve_triple_async) publishes two more forward values per separator variable
    into slots of their own: the publish entries behind those of the first right-hand side."""
    fused, levels = lmi_pair(K, n, branching, overlap, padded, seed=171)
    bs, cs = 0.9, 0.8
    for rep in range(3):  # (both sets of the extra hand-off slots)
        for k in (fused, levels):
            k.assemble()
        assert fused.L.cxk_triple_supported(fused.h) == 1  # (directly behind cxk_assemble)
        fused._check(fused.L.cxk_factor_solve_triple_async(fused.h, bs, cs), "cxk_factor_solve_triple_async")
        levels.factor_solve_async(-bs, cs, 0.0)
        assert fused.sync() and levels.sync()
        assert_factor_bits_direction_close(snapshot(fused), snapshot(levels))


def test_structural_fill_in_the_separator_rows():
    """A segmented chain of second-order cones carries deferred variables along as separator rows its constraints
    do not contain (position 255 in the record): their image entries point at the +0.0."""
    K = 8
    prob = syn.soc_problem(K=K, dim=10, m=10, overlap=2, seed=181)
    W = syn.soc_scaling_points(K, 10, seed=182)
    fused, levels = contexts(prob, W, "soc", CXK_CHAIN_SEGMENTS="4")
    assert fused.chain_segments() == 4 and levels.chain_segments() == 4
    # (14: the separator rows' positions in the own constraint, of the structure the factorization runs on)
    assert any((fused.get_list(14, e) < 0).any() for e in range(fused.K))
    all_launch_forms(fused, levels)


def test_leaves_in_both_frames_of_a_pair():
    """Hermitian cones over 24 variables and second-order cones over 10 in one tree: leaves of both kinds, each in
    its own frame of the pair, one image layout for both."""
    prob = syn.mixed_problem(K=30, seed=191)
    kinds = prob["kinds"]
    assert kinds[29] == "herm" and kinds[20] == "soc"  # (the nodes behind (K - 2) // 8 are leaves)
    W = syn.mixed_scaling_points(prob, seed=192)
    fused, levels = contexts(prob, W, "mixed")
    fa, fb = fused.fused_tree_frames()
    assert fa != fb
    all_launch_forms(fused, levels)


@pytest.mark.parametrize("where", ["leaf", "root"])
def test_a_failed_pivot_is_still_reported(where):
    """An indefinite scaling point on a leaf or on the root fails the solve, and the next solve with the valid point
    succeeds with the bits of a context that never failed (the pattern of test_gpu_elimination_step.py)."""
    K, n = 9, 20
    prob = syn.lmi_problem(K=K, n=n, m=M, branching=8, overlap=5, seed=81)
    W = syn.scaling_points(K, n, seed=82)
    c = K - 1 if where == "leaf" else 0  # (clique 0 is the root of the clique tree, the last clique one of its leaves)
    bad = W[c].copy()
    bad[0, 0] = -1e3

    k, fresh = build(prob, W), build(prob, W)
    assert k.fused_tree()
    k.set_W(c, bad)
    k.kkt_solve_async(0.7, 0.9, 0.8)
    assert not k.sync()
    k.set_W(c, W[c])
    for ctx in (k, fresh):
        ctx.kkt_solve_async(0.7, 0.9, 0.8)
        assert ctx.sync()
    for x, y in zip(snapshot(k), snapshot(fresh)):
        assert np.array_equal(x, y)


def test_dispatch_order_changes_no_bit():
    """Which workgroup takes which supernode (an eighth of the tree per XCD, depth first) moves records and images
    together: against CXK_FUSED_LEVEL_ORDER=1, the plain level order, every output bit is the same."""
    K, n = 73, 20
    prob = syn.lmi_problem(K=K, n=n, m=M, branching=8, overlap=5, seed=201)
    W = syn.scaling_points(K, n, seed=202)
    with environment(CXK_NO_FUSED_TREE=None, CXK_FUSED_LEVEL_ORDER=None):
        dealt = build(prob, W)
    with environment(CXK_NO_FUSED_TREE=None, CXK_FUSED_LEVEL_ORDER="1"):
        plain = build(prob, W)
    assert dealt.fused_tree() and plain.fused_tree()
    for mu in (0.7, 0.4, 0.9):
        for k in (dealt, plain):
            k.kkt_solve_async(mu, 0.9, 0.8)
            assert k.sync()
        assert_same_bits(snapshot(dealt), snapshot(plain))
    for k in (dealt, plain):
        k.assemble()
        assert k.L.cxk_triple_supported(k.h) == 1  # (directly behind cxk_assemble)
        k._check(k.L.cxk_factor_solve_triple_async(k.h, 0.9, 0.8), "cxk_factor_solve_triple_async")
        assert k.sync()
    assert_same_bits(snapshot(dealt), snapshot(plain))
