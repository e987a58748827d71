"""The fp64 MFMA GEMM (conex_amd/csrc/gemm_mfma.hip) on the operand layouts its callers pass, through
cxk_gemm_f64_layout: sub-blocks of a larger matrix, aliased operands, in-place updates, the transposed copy-out, raw
split partials, operands 8 bytes off alignment -- each on every kernel it can run on, inside an arena of poison
(tests/gemm_layout_cases.py: the reference in longdouble from the definition, the derived bound
(K + splits + 4) 2^-53 (|alpha| sum |a||b| + |beta C0|) inside the write set, unchanged bits outside it).

Every case asserts the route it was written for.  The routes here follow from three facts only: the LDS-DMA kernels
need even leading dimensions, even batch strides, 16-byte aligned operands, M, N, K >= 2 and an even K for an operand
that is contiguous along k; a stage of 32 k-values is taken from 512 k-values per split on; and at these batch sizes
(far fewer workgroups than the chip has CUs) the big tiles are reached only through the override.

A transposed copy-out of a lower-only product is refused by LaunchGemm (the kernels disagreed on what it holds: tiles
above the diagonal are skipped, tiles that run copied entries above it out; no caller asks for one), and so is a
copy-out through the ordered reduction, which never wrote one: both are asserted here as refusals.
"""
import copy

import numpy as np
import pytest

import gemm_layout_cases as glc
from conex_amd import kkt

pytestmark = pytest.mark.gpu

KERNELS = ("general", "dma64", "dma128x128", "dma128x64")   # what a test asks for: the override it sets


def eligible(c):
    even = all(c[k] % 2 == 0 for k in ("lda", "ldb", "sA1", "sA2", "sB1", "sB2", "offA", "offB"))
    k_contiguous = c["ta"] or not c["tb"]
    return even and min(c["M"], c["N"], c["K"]) >= 2 and not (k_contiguous and c["K"] % 2)


def written_for(c):
    """the route a case is written for, from the facts in the module's docstring"""
    if c["general"] or not eligible(c):
        return "general"
    assert max(c["splits"], 1) * c["batch"] * -(-c["M"] // 64) * -(-c["N"] // 64) < 256, "a case too big for this rule"
    gram = c["M"] <= 32 and c["N"] <= 32
    accumulating = c["beta"] != 0.0 and c["splits"] <= 1
    if c["tile"] in (128, 12864) and not gram and not accumulating:
        return "dma128x128" if c["tile"] == 128 else "dma128x64"
    per_split = -(-(-(-c["K"] // 16)) // max(c["splits"], 1)) * 16
    return "dma32" if per_split >= 512 else "dma16"


def on_kernel(c, kernel):
    c = dict(c)
    c["general"] = int(kernel == "general")
    c["tile"] = {"general": 0, "dma64": 64, "dma128x128": 128, "dma128x64": 12864}[kernel]
    return c


def run(c, n, family, seed=0, built=None):
    """build (unless given), run once, assert the route the case was written for, check; the figures are printed"""
    b = built if built is not None else glc.build(c, n, seed)
    after, route = kkt.gemm_f64_layout(b.arena, glc.fields_of(c), c["alpha"], c["beta"])
    assert route == written_for(c), (family, route, written_for(c), glc.fields_of(c))
    ratio = glc.check(b, after)
    print("%s %s M=%d N=%d K=%d splits=%d: worst error / bound %.3f" % (family, route, c["M"], c["N"], c["K"], c["splits"], ratio))
    return b, after, route


def run_on(cn, family, kernels, seed=0):
    """one build, one run per kernel asked for: the operands and the expectation are the same, the overrides differ"""
    c, n = cn
    b = glc.build(c, n, seed)
    for k in kernels:
        bk = copy.copy(b)
        bk.case = c if k == "natural" else on_kernel(c, k)
        run(bk.case, n, family, seed, built=bk)


ALL = ("natural", "general", "dma128x128", "dma128x64")


# ---------------------------------------------------------------------------------------------------------------
# caller patterns
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [141, 142])
@pytest.mark.parametrize("nb", [32, 13])
def test_panel_syrk_aliased_operands_in_one_matrix(ns, nb):
    for below in (1, 2, 31, 33, 64, 65, 109):
        c, n = glc.panel_syrk(ns, ns - below - nb, nb)
        want = "dma16" if ns % 2 == 0 and below % 2 == 0 else "general"
        assert written_for(c) == want
        run_on((c, n), "panel-syrk", ("natural", "general"), seed=below)


@pytest.mark.parametrize("below", [1, 33, 34, 65])
def test_panel_gemm_in_place_below_the_rows_it_reads(below):
    k0 = nb = 32
    for s in (1, 2, 17, 64, 66):
        c, n = glc.panel_gemm(below + k0 + nb, s, k0, nb)
        assert written_for(c) == ("dma16" if below == 34 and s >= 2 else "general")
        run_on((c, n), "panel-gemm", ("natural", "general"), seed=s)


@pytest.mark.parametrize("ns", [141, 142])
def test_separator_update_and_its_right_hand_side(ns):
    for s in (1, 2, 21, 45):
        c, n = glc.separator_update(ns, s)
        assert written_for(c) == ("dma16" if ns == 142 and s >= 2 else "general")
        run_on((c, n), "separator-update", ALL if s == 45 else ("natural", "general"), seed=s)
        c, n = glc.separator_rhs(ns, s)
        assert written_for(c) == "general"    # N = 1
        run_on((c, n), "separator-rhs", ("natural",), seed=s)


@pytest.mark.parametrize("n", [9, 10, 25, 64, 66])
def test_wide_product_with_transposed_copy_out(n):
    for m1 in (1, 3):
        for count in (1, 3):
            cn = glc.lmi_wide(n, m1, count)
            assert written_for(cn[0]) == ("general" if n % 2 else "dma16")
            run_on(cn, "lmi-wide", ALL if (m1, count) == (3, 1) else ("natural", "general"), seed=n + m1)


@pytest.mark.parametrize("n0", [5, 6, 16])
def test_folded_product_with_transposed_copy_out(n0):
    for d in (2, 4):
        cn = glc.lmi_folded(n0, d, 3, 2)
        assert written_for(cn[0]) == "dma16"
        run_on(cn, "lmi-folded", ALL, seed=n0 + d)


@pytest.mark.parametrize("m1", [1, 2, 17, 32, 33])
def test_gram_products_with_raw_partials(m1):
    K = 100                      # n = 10: ksteps = 7
    ksteps = 7
    for splits in (1, 2, ksteps - 1, ksteps, ksteps + 1):    # 6 and 8 leave EMPTY splits: zeros, not poison
        cn = glc.lmi_gram(K, m1, 2, splits)
        assert written_for(cn[0]) == ("general" if m1 == 1 else "dma16")
        run_on(cn, "lmi-gram", ALL if m1 == 33 else ("natural", "general"), seed=splits)
    assert [k0 == k1 for k0, k1 in glc.split_ranges(K, 6)] == [False] * 4 + [True] * 2
    cn = glc.lmi_gram(81, m1, 2, 3)     # n = 9: odd K
    assert written_for(cn[0]) == "general"
    run_on(cn, "lmi-gram", ("natural",))


@pytest.mark.parametrize("K,splits,want", [(496, 1, "dma16"), (512, 1, "dma32"), (992, 2, "dma16"), (1024, 2, "dma32"),
                                           (1026, 2, "dma32")])
def test_gram_products_at_the_stage_depth_switch(K, splits, want):
    for m1 in (17, 33):
        cn = glc.lmi_gram(K, m1, 2, splits)
        assert written_for(cn[0]) == want
        run_on(cn, "lmi-gram", ("natural",), seed=K)


@pytest.mark.parametrize("n", [9, 64, 65])
def test_square_products_with_a_batch_stride_of_two_matrices(n):
    cn = glc.lmi_aug(n, 2)
    assert written_for(cn[0]) == ("dma16" if n == 64 else "general")
    run_on(cn, "lmi-aug", ALL if n == 64 else ("natural",), seed=n)


@pytest.mark.parametrize("n", [8, 9])
def test_operands_eight_bytes_off_alignment(n):
    for m in (1, 8):
        for cn in (glc.quad_qa1(n, m, 2), glc.quad_gram(n, m, 2, True), glc.quad_gram(n, m, 2, False)):
            assert written_for(cn[0]) == "general"
            run_on(cn, "quad-constants", ("natural",), seed=n + m)


@pytest.mark.parametrize("n", [12, 64])
def test_factored_slack_accumulates(n):
    for dR in (2, 3, 8):
        cn = glc.factored_slack(n, dR, 2)
        assert written_for(cn[0]) == "dma16"
        run_on(cn, "factored-slack", ("natural", "general"), seed=dR)
    for dR, d in ((2, 2), (8, 2), (8, 4)):
        cn = glc.factored_slack(n, dR, 2, d=d)
        assert written_for(cn[0]) == "dma16"
        run_on(cn, "factored-slack", ALL, seed=dR + d)


@pytest.mark.parametrize("ln", [30, 31, 514])
def test_gram_lower_with_the_ordered_reduction(ln):
    for m in (2, 33, 64, 65):
        for splits in ((1, 2) if ln == 514 else (2,)):
            cn = glc.gram_lower(ln, m, 2, splits, alpha=2.0)
            want = "general" if ln == 31 else ("dma32" if (ln, splits) == (514, 1) else "dma16")
            assert written_for(cn[0]) == want
            run_on(cn, "gram-lower", ALL if m == 65 else ("natural", "general"), seed=m)


# ---------------------------------------------------------------------------------------------------------------
# each kernel at its tile edges
# ---------------------------------------------------------------------------------------------------------------
SIDES = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129)
DEPTHS = (1, 2, 15, 16, 17, 31, 32, 34)
# Every value of each, paired with one small (2) and one straddling (65; K: 34) value of the others.  Beside each value
# stands the route the shape is written for on the LDS-DMA kernels, as a literal: "small" = gemm_f64_dma<16> whatever
# tile is forced (at most 32 x 32), "forced" = the kernel the test forces (gemm_f64_dma<16> when that is the 64 x 64
# one), "general" = a side or depth of 1, "odd" = an odd K: general unless both operands are contiguous along m
# (no ta, tb), where it is what the even depths beside it are.
_SMALL_SIDE = {1: "general", 2: "small", 15: "small", 16: "small", 17: "small", 63: "forced", 64: "forced", 65: "forced",
               127: "forced", 128: "forced", 129: "forced"}
_WIDE_SIDE = {1: "general", 2: "forced", 15: "forced", 16: "forced", 17: "forced", 63: "forced", 64: "forced", 65: "forced",
              127: "forced", 128: "forced", 129: "forced"}
_SMALL_DEPTH = {1: "general", 2: "small", 15: "odd", 16: "small", 17: "odd", 31: "odd", 32: "small", 34: "small"}
_WIDE_DEPTH = {1: "general", 2: "forced", 15: "odd", 16: "forced", 17: "odd", 31: "odd", 32: "forced", 34: "forced"}
FAMILIES = (
    ("M beside small N, K", lambda v: (v, 2, 2), _SMALL_SIDE, "small"),
    ("M beside straddling N, K", lambda v: (v, 65, 34), _WIDE_SIDE, "forced"),
    ("N beside small M, K", lambda v: (2, v, 2), _SMALL_SIDE, "small"),
    ("N beside straddling M, K", lambda v: (65, v, 34), _WIDE_SIDE, "forced"),
    ("K beside small M, N", lambda v: (2, 2, v), _SMALL_DEPTH, "small"),
    ("K beside straddling M, N", lambda v: (65, 65, v), _WIDE_DEPTH, "forced"),
)
assert all(set(t) == set(SIDES) for _, _, t, _ in FAMILIES[:4]) and all(set(t) == set(DEPTHS) for _, _, t, _ in FAMILIES[4:])


def literal_route(kernel, word, even_word, ta, tb):
    if kernel == "general":
        return "general"
    if word == "odd":
        word = even_word if (ta, tb) == (0, 1) else "general"
    return {"general": "general", "small": "dma16", "forced": "dma16" if kernel == "dma64" else kernel}[word]


@pytest.mark.parametrize("ta,tb", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("kernel", KERNELS)
def test_tile_edges_on_padded_operands(kernel, ta, tb):
    routes = set()
    for name, shape, table, even_word in FAMILIES:
        for v, word in table.items():
            M, N, K = shape(v)
            # the general kernel takes both paddings as they come; the others get the one of rows + 2 / rows + 3 that is even
            for pad in ((2, 3) if kernel == "general" else ("even",)):
                c, n = glc.plain(M, N, K, ta, tb, pad=pad, batch=2)
                route = run(on_kernel(c, kernel), n, "tile-edges", seed=M + N + K)[2]
                assert route == literal_route(kernel, word, even_word, ta, tb), (name, v, route)
                routes.add(route)
    want = {"general": {"general"}, "dma64": {"general", "dma16"}, "dma128x128": {"general", "dma16", "dma128x128"},
            "dma128x64": {"general", "dma16", "dma128x64"}}[kernel]
    assert routes == want     # (dma16 under a big-tile override: the products of at most 32 x 32)


@pytest.mark.parametrize("ta,tb", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_long_k_on_the_deep_stage_kernel(ta, tb):
    for M, N, K in ((65, 33, 512), (17, 130, 546)):
        c, n = glc.plain(M, N, K, ta, tb, pad="even", batch=2)
        assert run(on_kernel(c, "dma64"), n, "tile-edges", seed=K)[2] == "dma32"


@pytest.mark.parametrize("kernel", KERNELS)
def test_accumulate_split_and_strides_per_kernel(kernel):
    # beta != 0 with alpha: on the big tiles only through splits (the reduction applies beta)
    c, n = glc.plain(130, 70, 100, 0, 1, pad="even", batch=2, alpha=-0.75, beta=1.25)
    assert run(on_kernel(c, kernel), n, "accumulate")[2] == ("general" if kernel == "general" else "dma16")
    for ta, tb in ((1, 0), (0, 1)):
        c, n = glc.plain(130, 130, 1026 if ta else 200, ta, tb, pad="even", splits=3, alpha=-0.75, beta=1.25)
        want = {"general": "general", "dma64": "dma16"}.get(kernel, kernel)
        assert run(on_kernel(c, kernel), n, "accumulate-split")[2] == want
        c, n = glc.plain(130, 130, 200, ta, tb, pad="even", splits=3, ordered=0, lower_only=1, batch=2)
        assert run(on_kernel(c, kernel), n, "raw-split")[2] == want
    # inner = 2: batch member z = (z / 2, z % 2) with a stride per level and operand, the transposed copy included
    c, n = glc.plain(66, 130, 34, 0, 0, pad="even", batch=4, inner=2, ct=True, alpha=0.5)
    assert run(on_kernel(c, kernel), n, "inner")[2] == {"general": "general", "dma64": "dma16"}.get(kernel, kernel)
    # lower_only on a full (not square) and on a compact (square) grid, one and several tiles a side
    for M, N in ((130, 66), (2, 2), (64, 64), (65, 65), (129, 129), (200, 200)):
        c, n = glc.plain(M, N, 34, 0, 1, pad="even", batch=2, lower_only=1, alpha=-1.0, beta=1.0)
        run(on_kernel(c, kernel), n, "lower-only")
        c, n = glc.plain(M, N, 34, 1, 0, pad="even", batch=3, lower_only=1)
        run(on_kernel(c, kernel), n, "lower-only")


@pytest.mark.parametrize("kernel", KERNELS)
def test_transposed_copy_out_refusals(kernel):
    c, n = glc.plain(66, 66, 34, 0, 0, pad="even", ct=True, lower_only=1)
    with pytest.raises(RuntimeError):
        kkt.gemm_f64_layout(glc.build(c, n).arena, glc.fields_of(on_kernel(c, kernel)))
    kkt.gemm_f64_layout(glc.build(c, n).arena, glc.fields_of(on_kernel(dict(c, lower_only=0), kernel)))   # (the layout itself is fine)
    c, n = glc.plain(66, 66, 34, 0, 0, pad="even", ct=True, splits=2)
    with pytest.raises(RuntimeError):
        kkt.gemm_f64_layout(glc.build(c, n).arena, glc.fields_of(on_kernel(c, kernel)))
    # raw partials with a copy-out asked for: the kernels write partials only, and nothing else
    c = dict(c, ordered=0)
    bb = glc.build(dict(c, offCt=-1), n)
    after, _ = kkt.gemm_f64_layout(bb.arena, glc.fields_of(on_kernel(c, kernel)))
    glc.check(bb, after)


def test_layouts_that_leave_the_arena_are_refused_before_any_launch():
    c, n = glc.plain(17, 9, 5, 0, 0, pad=2, batch=2, ct=True)
    b = glc.build(c, n)
    kkt.gemm_f64_layout(b.arena, glc.fields_of(c))
    for change in (dict(offC=n - 19 * 8 - 16), dict(sA1=n), dict(lda=16), dict(ldc=n), dict(offCt=n - 9), dict(sTb=n, ctb=2),
                   dict(batch=40), dict(offA=-1), dict(sB1=-2), dict(K=n), dict(splits=2), dict(splits=2, offPart=n - 5, sCs=4),
                   dict(inner=2 ** 32), dict(inner=0), dict(tile=7), dict(batch=2 ** 24, sC1=1), dict(splits=2 ** 24, offPart=0, sCs=1)):
        with pytest.raises(RuntimeError):
            kkt.gemm_f64_layout(b.arena, glc.fields_of(dict(c, **change)))


# ---------------------------------------------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
def test_packed_and_padded_layouts_give_the_same_bits(kernel):
    for (M, N, K, ta, tb, kw) in ((130, 66, 36, 0, 0, {}), (66, 130, 36, 1, 0, {}), (64, 64, 100, 0, 1, dict(alpha=-1.0, beta=1.0)),
                                  (128, 130, 40, 1, 1, dict(splits=2)), (30, 30, 64, 1, 0, dict(lower_only=1))):
        cp, n_p = glc.plain(M, N, K, ta, tb, pad=0, batch=2, **kw)
        cq, n_q = glc.plain(M, N, K, ta, tb, pad=4, batch=2, **kw)
        bp, after_p, rp = run(on_kernel(cp, kernel), n_p, "bits")
        cqk = on_kernel(cq, kernel)
        bq = glc.build(cqk, n_q, like=bp)
        _, after_q, rq = run(cqk, n_q, "bits", built=bq)
        assert rp == rq
        for z in range(2):
            got_p, got_q = glc.logical(bp, after_p, z)[bp.mask], glc.logical(bq, after_q, z)[bq.mask]
            assert np.array_equal(got_p.view(np.uint64), got_q.view(np.uint64)), (kernel, M, N, K, z)


@pytest.mark.parametrize("n", [25, 64, 66])
def test_wide_product_gives_the_bits_of_separate_products(n):
    """kernels_lmi_large.hip.h:816-821: W against [A_1 .. A_m C] side by side is the same products in the same k order
    as m + 1 products of n x n."""
    m1 = 3
    for kernel in ("natural", "general"):
        c, total = glc.lmi_wide(n, m1, 1)
        if kernel == "general":
            c = on_kernel(c, "general")
        b, after, route = run(c, total, "wide-bits", seed=n)
        nn = n * n
        sep = glc.case(M=n, N=n, K=n, batch=m1, offA=c["offA"], lda=n, sA1=0, offB=c["offB"], ldb=n, sB1=nn,
                       offC=c["offC"], ldc=n, sC1=nn, general=c["general"])
        after_s, route_s = kkt.gemm_f64_layout(b.arena, glc.fields_of(sep))
        assert route_s == route == written_for(sep)
        pt = slice(c["offC"], c["offC"] + m1 * nn)
        assert np.array_equal(after[pt].view(np.uint64), after_s[pt].view(np.uint64))
        assert np.isfinite(after_s[pt]).all()
