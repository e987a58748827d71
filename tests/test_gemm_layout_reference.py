"""tests/gemm_layout_cases.py on the CPU: the builder against a triple loop, the caller-pattern cases against the
GemmArgs their call sites state, and the write-set mask and the poison through a host round trip."""
import os
import re

import numpy as np
import pytest

import gemm_layout_cases as glc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "conex_amd", "csrc")


def triple_loop(c, arena):
    """C, Ct and the partials from the definition, one scalar at a time, in longdouble; returns {arena index: value}"""
    ld = np.longdouble
    out_c, out_t, out_p = {}, {}, {}
    ranges = glc.split_ranges(c["K"], c["splits"])
    for z in range(c["batch"]):
        b1, b2 = divmod(z, c["inner"])
        a0 = c["offA"] + b1 * c["sA1"] + b2 * c["sA2"]
        b0 = c["offB"] + b1 * c["sB1"] + b2 * c["sB2"]
        c0 = c["offC"] + b1 * c["sC1"] + b2 * c["sC2"]
        for m in range(c["M"]):
            for n in range(c["N"]):
                if c["lower_only"] and m < n:
                    continue
                terms = []
                for k in range(c["K"]):
                    a = arena[a0 + (k + m * c["lda"] if c["ta"] else m + k * c["lda"])]
                    b = arena[b0 + (n + k * c["ldb"] if c["tb"] else k + n * c["ldb"])]
                    terms.append(ld(a) * ld(b))
                acc = sum(terms, ld(0))
                at = c0 + m + n * c["ldc"]
                old = ld(arena[at]) if c["beta"] != 0 else ld(0)
                out_c[at] = ld(c["alpha"]) * acc + ld(c["beta"]) * old
                if c["offCt"] >= 0:
                    t0 = c["offCt"] + b1 * c["sT1"] + b2 * c["sT2"]
                    blk = (n // c["ctb"]) * c["sTb"] if c["ctb"] > 0 else 0
                    out_t[t0 + n + m * c["ldct"] + blk] = ld(c["alpha"]) * acc
                if c["splits"] > 1:
                    for s, (k0, k1) in enumerate(ranges):
                        out_p[c["offPart"] + (c0 - c["offC"]) + s * c["sCs"] + m + n * c["ldc"]] = sum(terms[k0:k1], ld(0))
    return out_c, out_t, out_p


TINY = [
    glc.plain(3, 2, 5, False, False, pad=2),
    glc.plain(3, 4, 2, True, False, pad=3, batch=2, alpha=-0.5, beta=2.0),
    glc.plain(4, 4, 3, False, True, pad=0, lower_only=1, beta=1.0, alpha=-1.0),
    glc.plain(2, 3, 4, True, True, pad=1, batch=4, inner=2, ct=True, alpha=3.0),
    glc.plain(3, 3, 40, True, False, pad=0, splits=3, lower_only=1, batch=2),
    glc.plain(2, 2, 20, False, False, pad=0, splits=4, ordered=0),        # an empty split among them
    glc.lmi_wide(3, 2, 2),
    glc.lmi_folded(2, 2, 2, 2),
    glc.panel_syrk(9, 2, 3),
    glc.panel_gemm(9, 2, 2, 3),
]


@pytest.mark.parametrize("i", range(len(TINY)))
def test_builder_equals_the_triple_loop(i):
    c, n = TINY[i]
    b = glc.build(c, n, seed=i)
    out_c, out_t, out_p = triple_loop(c, b.arena)
    A, B, C, Ct, P = b.idx
    raw = c["splits"] > 1 and not c["ordered"]
    tol = 4 * 2.0 ** -63 * (c["K"] + 2)   # two longdouble summation orders of at most K terms below 1 (+ alpha, beta < 4)
    seen = set()
    for z in range(c["batch"]):
        want = glc.expected_c(b, z)
        for m in range(c["M"]):
            for n_ in range(c["N"]):
                if not b.mask[m, n_]:
                    continue
                at = int(C[z][m, n_])
                assert abs(out_c[at] - want[m, n_]) <= tol * 4
                seen.add(at)
                if Ct:
                    assert abs(out_t[int(Ct[z][m, n_])] - np.longdouble(c["alpha"]) * b.prod[z][m, n_]) <= tol * 4
                    seen.add(int(Ct[z][m, n_]))
                for s in range(c["splits"] if c["splits"] > 1 else 0):
                    assert abs(out_p[int(P[z][s][m, n_])] - b.part[z][s][m, n_]) <= tol
                    seen.add(int(P[z][s][m, n_]))
    # the write set is exactly the set of elements the definition assigns (C itself is not written by a raw-partial call)
    expect = set(out_t) | set(out_p) | (set() if raw else set(out_c))
    assert set(np.flatnonzero(b.written).tolist()) == expect
    assert expect <= seen
    assert len(glc.split_ranges(20, 4)) == 4 and glc.split_ranges(20, 4)[2] == (20, 20)


def test_arena_is_poison_everywhere_but_operands_and_an_accumulated_c():
    c, n = glc.plain(5, 3, 4, False, False, pad=3, batch=2, beta=1.0)
    b = glc.build(c, n)
    A, B, C, Ct, P = b.idx
    finite = np.zeros(n, bool)
    for idx in A + B + C:
        finite[idx.ravel()] = True
    assert np.isfinite(b.arena[finite]).all() and glc.is_poison(b.arena[~finite]).all()
    assert glc.is_poison(b.arena[:glc.GUARD]).all() and glc.is_poison(b.arena[-glc.GUARD:]).all()
    # padding rows between rows and ld, and the gap between the batch members
    assert glc.is_poison(b.arena[c["offA"] + 5:c["offA"] + 8]).all()
    assert glc.is_poison(b.arena[c["offA"] + c["lda"] * 4:c["offA"] + c["sA1"]]).all()
    # beta == 0: the old C is poison too; lower_only with beta != 0: finite inside the mask only
    c0, n0 = glc.plain(5, 3, 4, False, False, pad=3)
    b0 = glc.build(c0, n0)
    assert glc.is_poison(b0.arena[b0.idx[2][0]]).all()
    cl, nl = glc.plain(4, 4, 2, False, True, lower_only=1, beta=1.0)
    bl = glc.build(cl, nl)
    old = bl.arena[bl.idx[2][0]]
    assert np.isfinite(old[bl.mask]).all() and glc.is_poison(old[~bl.mask]).all()
    # every region has at least GUARD doubles of poison before and after it
    for off in (c["offA"], c["offB"], c["offC"]):
        assert glc.is_poison(b.arena[off - glc.GUARD:off]).all()


def test_mask_and_poison_survive_a_host_round_trip():
    c, n = glc.plain(6, 6, 3, False, True, pad=2, lower_only=1, beta=1.0, alpha=-1.0)
    b = glc.build(c, n)
    after = np.frombuffer(bytes(memoryview(b.arena.copy())), dtype=np.float64).copy()   # what a copy out and back does
    assert np.array_equal(after.view(np.uint64), b.before)
    assert (after.view(np.uint64)[~np.isfinite(after)] & np.uint64(0xFFFFFFFF) ==
            np.flatnonzero(~np.isfinite(after)).astype(np.uint64)).all()
    # an exact result passes; each kind of damage is caught
    exact = after.copy()
    exact[b.idx[2][0][b.mask]] = glc.expected_c(b, 0)[b.mask].astype(np.float64)
    assert glc.check(b, exact) <= 1.0
    for at, value in ((int(b.idx[2][0][0, 1]), 0.5),            # a store above the diagonal
                      (c["offC"] - 1, 0.0),                      # a store into the guard
                      (c["offC"] + 6, float("nan"))):            # a padding row: another NaN than the poison
        bad = exact.copy()
        bad[at] = value
        with pytest.raises(AssertionError):
            glc.check(b, bad)
    bad = exact.copy()
    at = int(b.idx[2][0][3, 1])
    bad[at] = bad[at] * (1 + 2.0 ** -44)   # wrong in the ninth digit from the end: outside (K + 5) 2^-53
    with pytest.raises(AssertionError):
        glc.check(b, bad)
    bad = after.copy()                      # beta C0 left out / the old C never replaced
    with pytest.raises(AssertionError):
        glc.check(b, bad)


def _source(site):
    name, lines = site.split(":")
    lo, hi = (int(x) for x in lines.split("-"))
    with open(os.path.join(CSRC, name)) as f:
        text = f.read().split("\n")
    return re.sub(r"\s+", " ", " ".join(text[lo - 1:hi]))


def test_caller_patterns_state_what_their_call_sites_state():
    """Each caller-pattern case against the text of the call site it cites: the statement that sets every GemmArgs
    field must stand in the cited lines as the case's docstring quotes it, and the case must carry those values."""
    ns, k0, nb, s = 141, 32, 32, 17
    below = ns - k0 - nb
    c, _ = glc.panel_syrk(ns, k0, nb)
    src = _source(c["site"])
    assert "const double* L21 = D + (k0 + nb) + (size_t)k0 * ns;" in src
    assert "BigGemm(below, below, nb, L21, ns, L21, ns, D + (k0 + nb) + (size_t)(k0 + nb) * ns, ns, -1.0, 1.0, 1);" in src
    assert "LaunchGemm(g1, false, true, 1, st)" in src
    D = c["offA"] - (k0 + nb) - k0 * ns
    assert (c["M"], c["N"], c["K"], c["ta"], c["tb"]) == (below, below, nb, 0, 1)
    assert c["offA"] == c["offB"] and c["lda"] == c["ldb"] == c["ldc"] == ns
    assert c["offC"] == D + (k0 + nb) + (k0 + nb) * ns and (c["alpha"], c["beta"], c["lower_only"]) == (-1.0, 1.0, 1)
    # (BigGemm's argument order: kernels_kkt_big.hip.h, the function above BigSupernodeSweep)
    big = _source("kernels_kkt_big.hip.h:385-407")
    assert re.search(r"BigGemm\(int M, int N, int K, const double\* A, int(64_t)? lda, const double\* B, int(64_t)? ldb, "
                     r"double\* C, int(64_t)? ldc, double alpha, double beta, int lower_only\)", big), big

    c, _ = glc.panel_gemm(ns, s, k0, nb)
    src = _source(c["site"])
    assert "BigGemm(below, s, nb, L21, ns, B + k0, ns, B + k0 + nb, ns, -1.0, 1.0, 0);" in src
    assert "LaunchGemm(g2, false, false, 1, st)" in src
    assert (c["M"], c["N"], c["K"], c["ta"], c["tb"]) == (below, s, nb, 0, 0)
    assert c["offC"] == c["offB"] + nb and c["lda"] == c["ldb"] == c["ldc"] == ns and c["lower_only"] == 0

    c, _ = glc.separator_update(ns, s)
    src = _source(c["site"])
    assert "BigGemm(s, s, ns, B, ns, B, ns, U, s, 1.0, 0.0, 0);" in src and "LaunchGemm(g, true, false, 1, st)" in src
    assert (c["M"], c["N"], c["K"], c["ta"], c["tb"], c["ldc"]) == (s, s, ns, 1, 0, s) and c["offA"] == c["offB"]

    c, _ = glc.separator_rhs(ns, s)
    src = _source(c["site"])
    assert "BigGemm(s, 1, ns, B, ns, b, ns, t, s, 1.0, 0.0, 0);" in src and "LaunchGemm(g, true, false, 1, st)" in src
    assert (c["M"], c["N"], c["K"], c["ta"], c["tb"], c["ldc"]) == (s, 1, ns, 1, 0, s)

    n, m1, count = 10, 3, 2
    nn = n * n
    c, _ = glc.lmi_wide(n, m1, count)
    src = _source(c["site"])
    for stmt in ("a.M = n;", "a.N = n * m1;", "a.K = n;", "a.A = g.W;", "a.lda = n;", "a.sA1 = nn;", "a.B = g.A;",
                 "a.ldb = n;", "a.sB1 = g.a_stride;", "a.C = ws.PT;", "a.ldc = n;", "a.sC1 = m1 * nn;", "a.Ct = ws.P;",
                 "a.ldct = n;", "a.sT1 = m1 * nn;", "a.ctb = n;", "a.sTb = nn - n;", "a.beta = 0.0;", "a.splits = 1;",
                 "LaunchGemm(a, false, false, g.count, st)"):
        assert stmt in src, stmt
    assert (c["M"], c["N"], c["K"], c["lda"], c["sA1"], c["ldb"], c["ldc"], c["sC1"]) == (n, n * m1, n, n, nn, n, n, m1 * nn)
    assert (c["ldct"], c["sT1"], c["ctb"], c["sTb"], c["batch"]) == (n, m1 * nn, n, nn - n, count)

    n0, d = 6, 2
    n = n0 * d
    nn, per = n * n, n0 * n
    c, _ = glc.lmi_folded(n0, d, m1, count)
    src = _source(c["site"])
    for stmt in ("a.N = n0 * m1;", "a.B = ws.Aleft;", "a.sB1 = per * m1;", "a.sC1 = stride;", "a.ldct = n0;", "a.sT1 = stride;",
                 "a.ctb = n0;", "a.sTb = per - n0;", "LaunchGemm(a, false, false, g.count, st)"):
        assert stmt in src, stmt
    assert (c["M"], c["N"], c["K"], c["sB1"], c["sC1"]) == (n, n0 * m1, n, per * m1, m1 * nn)
    assert (c["ldct"], c["sT1"], c["ctb"], c["sTb"]) == (n0, m1 * nn, n0, per - n0)

    c, _ = glc.lmi_gram(nn, m1, count, 3)
    src = _source(c["site"])
    for stmt in ("a.M = a.N = m1;", "a.K = (int)nn;", "a.lda = nn;", "a.sA1 = m1 * nn;", "a.ldb = nn;", "a.sB1 = m1 * nn;",
                 "a.ldc = m1;", "a.sC1 = (int64_t)m1 * m1;", "a.lower_only = 1;", "a.sCs = (int64_t)g.count * m1 * m1;",
                 "if (split) a.C = ws.part;", "LaunchGemm(a, true, false, g.count, st)"):
        assert stmt in src, stmt
    src = _source("kernels_lmi_large.hip.h:788-807")
    for stmt in ("a.K = (int)per;", "a.lda = per;", "a.sA1 = stride;", "a.ldb = per;", "a.sB1 = stride;",
                 "if (a.splits > 1) a.C = ws.part;", "LaunchGemm(a, true, false, g.count, st)"):
        assert stmt in src, stmt
    assert (c["M"], c["N"], c["K"], c["ta"], c["tb"], c["lda"], c["ldb"], c["sA1"]) == (m1, m1, nn, 1, 0, nn, nn, m1 * nn)
    assert (c["ldc"], c["sC1"], c["sCs"], c["lower_only"], c["ordered"]) == (m1, m1 * m1, count * m1 * m1, 1, 0)

    c, _ = glc.lmi_aug(n, count)
    src = _source(c["site"])
    assert "SquareGemm(n, aug + nn, 2 * nn, g.W, nn, EW, nn);" in src and "LaunchGemm(c, false, false, count, st)" in src
    assert (c["sA1"], c["sB1"], c["sC1"], c["lda"]) == (2 * nn, nn, nn, n)

    n, m = 9, 8
    c, _ = glc.quad_qa1(n, m, count)
    src = _source(c["site"])
    assert "const double* A1 = g.A.p + (size_t)b0 * len * m + 1;" in _source("cone_quad.hip:177-177")
    for stmt in ("a.M = n;", "a.N = m;", "a.K = n;", "a.lda = n;", "a.B = A1;", "a.ldb = len;", "a.sB1 = (int64_t)len * m;",
                 "a.ldc = n;", "a.sC1 = (int64_t)n * m;", "LaunchGemm(a, false, false, nb, ctx->stream)"):
        assert stmt in src, stmt
    assert (c["ldb"], c["sB1"], c["offB"] & 1) == (n + 1, (n + 1) * m, 1)
    c, _ = glc.quad_gram(n, m, count, True)
    src = _source(c["site"])
    for stmt in ("a.M = a.N = m;", "a.K = n;", "a.A = A1;", "a.lda = len;", "a.sA1 = (int64_t)len * m;", "a.ldc = m;",
                 "LaunchGemm(a, true, false, nb, ctx->stream)"):
        assert stmt in src, stmt
    assert (c["lda"], c["sA1"], c["offA"] & 1, c["ldb"]) == (n + 1, (n + 1) * m, 1, n)

    n, dR = 12, 3
    c, _ = glc.factored_slack(n, dR, count)
    src = _source(c["site"])
    for stmt in ("a.M = a.N = n, a.K = d * R;", "a.A = f.Fs, a.lda = n, a.sA1 = nf;", "a.B = f.F, a.ldb = n, a.sB1 = nf;",
                 "a.C = S, a.ldc = n, a.sC1 = nn;", "a.beta = 1.0;", "LaunchGemm(a, false, true, g.count, st)", "a.N = n / d;",
                 "a.C = T, a.sC1 = (int64_t)n * (n / d);", "a.beta = 0.0;"):
        assert stmt in src, stmt
    assert (c["M"], c["N"], c["K"], c["tb"], c["sA1"], c["sC1"], c["beta"]) == (n, n, dR, 1, n * dR, n * n, 1.0)
    c, _ = glc.factored_slack(n, 4, count, d=2)
    assert (c["N"], c["sC1"], c["beta"]) == (n // 2, n * (n // 2), 0.0)

    ln, m = 30, 33
    c, _ = glc.gram_lower(ln, m, count, 2, alpha=2.0)
    src = _source(c["site"])
    for stmt in ("a.M = a.N = m;", "a.K = len;", "a.A = a.B = WA + (size_t)b0 * len * m;", "a.lda = a.ldb = len;",
                 "a.sA1 = a.sB1 = (int64_t)len * m;", "a.ldc = m;", "a.sC1 = mm;", "a.alpha = alpha;", "a.lower_only = 1;",
                 "a.sCs = (int64_t)std::min(cnt, kMaxBatch) * mm;", "LaunchGemmSplitK(a, true, false, nb, w.part.p, st)"):
        assert stmt in src, stmt
    assert c["offA"] == c["offB"] and (c["lda"], c["sA1"], c["sCs"], c["ordered"]) == (ln, ln * m, count * m * m, 1)
