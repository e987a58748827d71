"""The software-pipelined elimination step of the two-row register shapes (dense_elim.hip.h):
the mirror of the next pivot column taken from the unscaled column ahead of the reciprocal square root's
chain, the mask of the pivot lane compared at its step, the chain interleaved with the multiply-adds.

Exact-fit frames: BuildPlans picks the tightest compiled pair of register frames for the whole-tree launch
(15 + 5 columns under a root of 20: <16, 5> and <20, 0> instead of <16, 8> and <24, 0>);
CXK_FUSED_PADDED_FRAMES=1, read when the plans are built, keeps the padded pair.  Padding contributes exact
zeros and unit pivots, so the two choices must agree in EVERY bit of every output.

Same fma chains on the same values, so the whole-tree launch must still produce the level kernels'
(CXK_NO_FUSED_TREE=1) factor, AW / AQc and scalars BIT FOR BIT and their direction to 1e-13, as
test_gpu_fused_tree.py asks -- here at the shapes where the recursion ends early (fewer columns than the
frame: the padding pivots are skipped), where it runs to its end (a full frame), and along a chain (every
supernode has one child).  Every launch form that runs the step is compared: the factor-and-solve, the
assemble / factor order of the interior-point loop, three right-hand sides, the two-launch form."""
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


def build(prob, W):
    k = syn.build(KktContext, prob, "lmi", device=0)
    for i in range(k.K):
        k.set_W(i, W[i])
    k.set_cost(prob["b"])
    return k


def contexts(prob, W, **env):
    """(whole-tree launch, level kernels) on the same problem and scaling points"""
    with environment(**env):
        with environment(CXK_NO_FUSED_TREE=None):
            fused = build(prob, W)
        with environment(CXK_NO_FUSED_TREE="1"):
            levels = build(prob, W)
    assert fused.fused_tree() and not levels.fused_tree()
    return fused, levels


def snapshot(k):
    AW, AQc, sc = k.residuals()
    return k.get_y().copy(), k.slab().copy(), AW, AQc, sc


def assert_factor_bits_direction_close(a, b):
    assert np.linalg.norm(a[0] - b[0]) <= 1e-13 * np.linalg.norm(b[0])
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y, equal_nan=True)


# 13 + 7 and (LMIs of order 12) 13 + 7 again in the <16, 8> frame, the root's 20 columns in <24, 0>: both
# recursions leave early; 16 + 4 fills <16, 8> (its last pivot's step reads a[15] itself as a DPP operand);
# a chain of six: every supernode but the leaf pulls from exactly one child
SHAPES = [(9, 20, 8, 7), (9, 12, 8, 7), (9, 8, 8, 4), (6, 20, 1, 5), (73, 20, 8, 5)]
# The frames each of them must run in.  The early-exit shapes (overlap 7) and the full frame ask for the padded pair
# by name, so that a pair compiled later does not change what they cover; the last two run the default, exact-fit pair.
PADDED = ((16, 8), (24, 0))
FRAMES = {7: ("1", PADDED), 4: ("1", PADDED), 5: (None, ((16, 5), (20, 0)))}


def fused_and_levels(prob, W, overlap, **env):
    switch, frames = FRAMES[overlap]
    fused, levels = contexts(prob, W, CXK_FUSED_PADDED_FRAMES=switch, **env)
    assert fused.fused_tree_frames() == frames
    return fused, levels


@pytest.mark.parametrize("K,n,branching,overlap", SHAPES)
def test_pipelined_step_equals_level_kernels(K, n, branching, overlap):
    prob = syn.lmi_problem(K=K, n=n, m=M, branching=branching, overlap=overlap, seed=51 + K + n)
    W = syn.scaling_points(K, n, seed=52)
    fused, levels = fused_and_levels(prob, W, overlap)
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


@pytest.mark.parametrize("K,n,branching,overlap", SHAPES[:4])
def test_pipelined_step_in_the_two_launch_form(K, n, branching, overlap):
    """CXK_FUSED_SPLIT=1: the way up as a launch of its own (right-hand side columns, pivots tested per step);
    it sweeps back down as the level kernels do, so the direction is the same bits too."""
    prob = syn.lmi_problem(K=K, n=n, m=M, branching=branching, overlap=overlap, seed=61 + K + n)
    W = syn.scaling_points(K, n, seed=62)
    fused, levels = fused_and_levels(prob, W, overlap, CXK_FUSED_SPLIT="1")
    for mu in (0.7, 0.4, 0.9):
        for k in (fused, levels):
            k.kkt_solve_async(mu, 0.9, 0.8)
            assert k.sync()
        for x, y in zip(snapshot(fused), snapshot(levels)):
            assert np.array_equal(x, y, equal_nan=True)


@pytest.mark.parametrize("K,n,branching,overlap", SHAPES[:4])
def test_pipelined_step_with_three_right_hand_sides(K, n, branching, overlap):
    """The triple launch (cxk_factor_solve_triple_async) runs the same step with three right-hand-side rows under
    the panel: its factor is the level kernels' bit for bit, its y = K^-1 (-bs b + cs AQc) theirs to rounding."""
    prob = syn.lmi_problem(K=K, n=n, m=M, branching=branching, overlap=overlap, seed=71 + K + n)
    W = syn.scaling_points(K, n, seed=72)
    fused, levels = fused_and_levels(prob, W, overlap)
    bs, cs = 0.9, 0.8
    for rep in range(3):  # (both sets of the extra hand-off slots)
        for k in (fused, levels):
            k.assemble()
        assert fused.L.cxk_triple_supported(fused.h) == 1  # (directly behind cxk_assemble)
        fused._check(fused.L.cxk_factor_solve_triple_async(fused.h, bs, cs), "cxk_factor_solve_triple_async")
        levels.factor_solve_async(-bs, cs, 0.0)
        assert fused.sync() and levels.sync()
        a, b = snapshot(fused), snapshot(levels)
        assert np.linalg.norm(a[0] - b[0]) <= 1e-12 * np.linalg.norm(b[0])  # (two solutions combined: test_gpu_triple.py)
        for x, y in zip(a[1:], b[1:]):
            assert np.array_equal(x, y, equal_nan=True)


@pytest.mark.parametrize("where", ["leaf", "root"])
def test_a_failed_pivot_is_still_reported(where):
    """The whole-tree launch judges the pivots by the NaNs they leave in the solution, the steps test nothing: an
    indefinite scaling point on a leaf or on the root fails the solve, and the next solve with the valid point
    succeeds with the bits of a context that never failed.  (The Schur block is quadratic in W, so W = -I would
    give the positive definite block of W = I: the point has ONE negative eigenvalue, as in
    test_gpu_lean_kernels.py.)"""
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


# ---- exact-fit frames against the padded ones: every comparison bit for bit ----------------------------------

def frame_pair(prob, W, **env):
    """(default frames, CXK_FUSED_PADDED_FRAMES=1) on the same problem and scaling points"""
    with environment(**env):
        with environment(CXK_FUSED_PADDED_FRAMES=None):
            tight = build(prob, W)
        with environment(CXK_FUSED_PADDED_FRAMES="1"):
            padded = build(prob, W)
    assert tight.fused_tree() and padded.fused_tree()
    return tight, padded


def assert_same_bits(a, b):
    for x, y in zip(snapshot(a), snapshot(b)):
        assert np.array_equal(x, y)


# root and eight leaves; three levels (a supernode with descendants AND a separator); a chain; the root alone -- no
# instance is compiled for <20, 0> alone, it keeps <24, 0> in both builds: that row exercises no exact-fit frame, it
# only holds that the frame choice leaves a single-supernode program as it was
FRAME_SHAPES = [(9, 8, ((16, 5), (20, 0))), (73, 8, ((16, 5), (20, 0))), (4, 1, ((16, 5), (20, 0))),
                (1, 8, ((24, 0), (24, 0)))]


@pytest.mark.parametrize("K,branching,frames", FRAME_SHAPES)
def test_exact_fit_frames_change_no_bit(K, branching, frames):
    prob = syn.lmi_problem(K=K, n=20, m=M, branching=branching, overlap=5, seed=91 + K)
    W = syn.scaling_points(K, 20, seed=92)
    tight, padded = frame_pair(prob, W)
    assert tight.fused_tree_frames() == frames
    assert padded.fused_tree_frames() == (((16, 8), (24, 0)) if K > 1 else ((24, 0), (24, 0)))
    for mu in (0.7, 0.4, 0.9, 0.55, 0.61):  # (five launches: both sets of hand-off slots)
        for k in (tight, padded):
            k.kkt_solve_async(mu, 0.9, 0.8)
            assert k.sync()
        assert_same_bits(tight, padded)
    for k in (tight, padded):
        k.assemble()
        k.factor_solve_async(-0.9, 0.8, 0.0)
        assert k.sync()
    assert_same_bits(tight, padded)
    # three right-hand sides (the entry of test_gpu_triple.py): y and the three solutions behind it
    for k in (tight, padded):
        k.assemble()
        assert k.L.cxk_triple_supported(k.h) == 1  # (directly behind cxk_assemble)
        k._check(k.L.cxk_factor_solve_triple_async(k.h, 0.9, 0.8), "cxk_factor_solve_triple_async")
        assert k.sync()
    assert_same_bits(tight, padded)
    for k in (tight, padded):
        k.solve_rhs(0.3, -0.2, 1.5)
        assert k.sync()
    assert np.array_equal(tight.get_y(), padded.get_y())


@pytest.mark.parametrize("K,branching", [(9, 8), (73, 8), (4, 1)])
def test_exact_fit_frames_in_the_two_launch_form(K, branching):
    prob = syn.lmi_problem(K=K, n=20, m=M, branching=branching, overlap=5, seed=95 + K)
    W = syn.scaling_points(K, 20, seed=96)
    tight, padded = frame_pair(prob, W, CXK_FUSED_SPLIT="1")
    assert tight.fused_tree_frames() == ((16, 5), (20, 0))
    for mu in (0.7, 0.4, 0.9):
        for k in (tight, padded):
            k.kkt_solve_async(mu, 0.9, 0.8)
            assert k.sync()
        assert_same_bits(tight, padded)
    for k in (tight, padded):
        k.solve_rhs(0.3, -0.2, 1.5)
        assert k.sync()
    assert np.array_equal(tight.get_y(), padded.get_y())


def test_a_failed_pivot_is_reported_in_either_frame_choice():
    K, n = 9, 20
    prob = syn.lmi_problem(K=K, n=n, m=M, branching=8, overlap=5, seed=81)
    W = syn.scaling_points(K, n, seed=82)
    for c in (K - 1, 0):  # a leaf, the root
        tight, padded = frame_pair(prob, W)
        bad = W[c].copy()
        bad[0, 0] = -1e3
        for k in (tight, padded):
            k.set_W(c, bad)
            k.kkt_solve_async(0.7, 0.9, 0.8)
            assert not k.sync()
            k.set_W(c, W[c])
            k.kkt_solve_async(0.7, 0.9, 0.8)
            assert k.sync()
        assert_same_bits(tight, padded)
