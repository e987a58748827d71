"""Cases for the fp64 MFMA GEMM (conex_amd/csrc/gemm_mfma.hip) on the operand layouts its callers pass.

A case is a dict over the fields of cxk_gemm_f64_layout (conex_amd.kkt.GEMM_LAYOUT_FIELDS, the GemmArgs of
kernels_gemm.hip.h with pointers as element offsets into ONE arena) plus alpha and beta.  build() lays the arena out:
operand entries uniform in (-1, 1); EVERYTHING else -- the padding rows between `rows` and `ld`, the gaps between
batch members, the guards, the old C wherever beta == 0, the partial buffers -- a quiet NaN whose payload holds the
element's own index (POISON | index), so that a value the kernel picked up from outside an operand, or a store
outside the write set, cannot pass for a plausible number.  Where beta != 0 the old C is finite inside the write
set and poison outside it.

The expectation is computed in numpy.longdouble (64-bit mantissa, asserted) straight from the definition,
  C(m, n) = alpha sum_k op(A)(m, k) op(B)(k, n) + beta C0(m, n),   Ct[n + m ldct + (n / ctb) sTb] = alpha sum_k ...,
through index arrays into the arena: nothing goes through any code of the library.

check() has two parts.  Inside the write set (C: m < M, n < N, and m >= n under lower_only; Ct: its image; the
partials: every split of every batch member over the same mask) the error of an element is at most
  (K + splits + 4) 2^-53 (|alpha| sum_k |a||b| + |beta C0|):
accumulating a length-K dot product in fp64 in any order rounds at most K times, the ordered reduction adds `splits`
roundings, alpha, beta and the final add the rest.  Outside the write set every arena element has the bits it had
before the call (compared as uint64: NaN payloads survive a copy).
"""
import numpy as np

assert np.finfo(np.longdouble).nmant >= 63, "numpy.longdouble is not the 64-bit-mantissa format the bound assumes"

GUARD = 64                          # doubles of poison before and after every region
POISON = 0x7FF8DEAD00000000         # quiet NaN; the low 32 bits carry the element's index
U = 2.0 ** -53
BK = 16                             # kGemmBK: a split is a whole number of steps of this many k

DEFAULTS = dict(ta=0, tb=0, batch=1, inner=1, lower_only=0, splits=1, ordered=1, tile=0, general=0,
                sA1=0, sA2=0, sB1=0, sB2=0, sC1=0, sC2=0, offCt=-1, ldct=0, sT1=0, sT2=0, ctb=0, sTb=0,
                offPart=-1, sCs=0, alpha=1.0, beta=0.0)


def case(**kw):
    c = dict(DEFAULTS)
    c.update(kw)
    return c


def poison(n):
    return (np.uint64(POISON) | np.arange(n, dtype=np.uint64)).view(np.float64)


def is_poison(x):
    return (np.asarray(x).view(np.uint64) >> np.uint64(32)) == np.uint64(POISON >> 32)


def split_ranges(K, splits):
    """k range of every split, as every kernel deals them: whole steps of BK, ceil(ksteps / splits) each."""
    ksteps = (K + BK - 1) // BK
    per = (ksteps + splits - 1) // splits
    return [(min(K, s * per * BK), min(K, (s + 1) * per * BK)) for s in range(splits)]


class Arena:
    """Lays regions one after the other with GUARD doubles of poison around each; returns their offsets."""

    def __init__(self):
        self.n = GUARD

    def take(self, length, odd=False):
        """offset of a new region of `length` doubles: 16-byte aligned (even), or 8 bytes off (odd)"""
        off = self.n + ((self.n & 1) != (1 if odd else 0))
        self.n = off + length + GUARD
        return off

    def cover_ct(self, c):
        """Lengthen the guard behind Ct so that a copy-out with its column bound dropped -- n running to the end of
        the widest tile, 128 columns, and on through further ctb blocks -- still lands in poison inside the arena,
        where check() sees it, and not outside the allocation."""
        n_max = -(-c["N"] // 128) * 128 - 1
        b1, b2 = divmod(c["batch"] - 1, c["inner"])
        end = (c["offCt"] + b1 * c["sT1"] + b2 * c["sT2"] + n_max + (c["M"] - 1) * c["ldct"] +
               ((n_max // c["ctb"]) * c["sTb"] if c["ctb"] > 0 else 0) + 1)
        self.n = max(self.n, end + GUARD)

    def total(self):
        return self.n + GUARD


class Built:
    pass


def indices(c):
    """Arena indices of op(A)(m, k), op(B)(k, n), C(m, n), Ct's image of (m, n) and the partials, per batch member."""
    M, N, K = c["M"], c["N"], c["K"]
    m = np.arange(M, dtype=np.int64)
    n = np.arange(N, dtype=np.int64)
    k = np.arange(K, dtype=np.int64)
    A, B, C, Ct, P = [], [], [], [], []
    for z in range(c["batch"]):
        b1, b2 = divmod(z, c["inner"])
        a0 = c["offA"] + b1 * c["sA1"] + b2 * c["sA2"]
        b0 = c["offB"] + b1 * c["sB1"] + b2 * c["sB2"]
        crel = b1 * c["sC1"] + b2 * c["sC2"]
        A.append(a0 + (k[None, :] + m[:, None] * c["lda"] if c["ta"] else m[:, None] + k[None, :] * c["lda"]))
        B.append(b0 + (n[None, :] + k[:, None] * c["ldb"] if c["tb"] else k[:, None] + n[None, :] * c["ldb"]))
        cidx = m[:, None] + n[None, :] * c["ldc"]
        C.append(c["offC"] + crel + cidx)
        if c["offCt"] >= 0:
            t0 = c["offCt"] + b1 * c["sT1"] + b2 * c["sT2"]
            blk = (n // c["ctb"]) * c["sTb"] if c["ctb"] > 0 else 0 * n
            Ct.append(t0 + n[None, :] + m[:, None] * c["ldct"] + blk[None, :])
        if c["splits"] > 1:
            P.append([c["offPart"] + crel + s * c["sCs"] + cidx for s in range(c["splits"])])
    return A, B, C, Ct, P


def build(c, arena_len, seed=0, like=None):
    """The arena before the call, the expectation and the write set of case `c`.  like: a Built of the same logical
    product in another layout, whose operand and old-C values this one takes over (for bit comparisons)."""
    rng = np.random.default_rng(seed)
    M, N, K, splits = c["M"], c["N"], c["K"], c["splits"]
    raw = splits > 1 and not c["ordered"]
    A, B, C, Ct, P = indices(c)
    for idx in A + B + C + Ct + [p for ps in P for p in ps]:
        assert idx.min() >= GUARD and idx.max() < arena_len - GUARD, "a case that leaves its arena's guards"
    arena = poison(arena_len)
    operand = np.zeros(arena_len, bool)
    for idx in A + B:
        operand[idx.ravel()] = True
    arena[operand] = rng.uniform(-1.0, 1.0, int(operand.sum()))
    if like is not None:
        for z in range(c["batch"]):
            arena[A[z]] = like.arena[like.idx[0][z]]
            arena[B[z]] = like.arena[like.idx[1][z]]
    mask = np.tril(np.ones((M, N), bool)) if c["lower_only"] else np.ones((M, N), bool)
    written = np.zeros(arena_len, bool)
    for z in range(c["batch"]):
        if not raw:
            written[C[z][mask]] = True
        if Ct:
            written[Ct[z][mask]] = True
        if splits > 1:
            for p in P[z]:
                written[p[mask]] = True
    assert not (written & operand).any(), "a case whose write set overlaps an operand it reads"
    if c["beta"] != 0.0 and not raw:
        for z in range(c["batch"]):
            arena[C[z][mask]] = rng.uniform(-1.0, 1.0, int(mask.sum())) if like is None else like.arena[like.idx[2][z][mask]]
    ld = np.longdouble
    b = Built()
    b.case, b.arena, b.before = c, arena, arena.view(np.uint64).copy()
    b.mask, b.written, b.idx = mask, written, (A, B, C, Ct, P)
    b.prod, b.mag, b.c0, b.part, b.part_mag = [], [], [], [], []
    for z in range(c["batch"]):
        a, bb = arena[A[z]].astype(ld), arena[B[z]].astype(ld)
        assert np.isfinite(a).all() and np.isfinite(bb).all()
        b.prod.append(a @ bb)
        b.mag.append(np.abs(a) @ np.abs(bb))
        c0 = np.zeros((M, N), ld)
        if c["beta"] != 0.0 and not raw:
            c0[mask] = arena[C[z][mask]].astype(ld)
        b.c0.append(c0)
        if splits > 1:
            b.part.append([a[:, k0:k1] @ bb[k0:k1, :] for k0, k1 in split_ranges(K, splits)])
            b.part_mag.append([np.abs(a[:, k0:k1]) @ np.abs(bb[k0:k1, :]) for k0, k1 in split_ranges(K, splits)])
    return b


def expected_c(b, z):
    c = b.case
    return np.longdouble(c["alpha"]) * b.prod[z] + np.longdouble(c["beta"]) * b.c0[z]


def bound_c(b, z):
    c = b.case
    return (c["K"] + c["splits"] + 4) * U * (abs(c["alpha"]) * b.mag[z] + np.abs(np.longdouble(c["beta"]) * b.c0[z]))


def worst(got, want, bound, mask):
    """largest error / bound over the mask (inf for a NaN or where a zero bound is missed); 0 for an exact match"""
    err = np.abs(got.astype(np.longdouble) - want)[mask]
    bd = bound[mask]
    ratio = np.where(err == 0, 0.0, err / np.where(bd > 0, bd, 1.0))
    ratio = np.where((bd <= 0) & (err != 0), np.inf, ratio)
    ratio = np.where(np.isnan(err), np.inf, ratio)
    return float(ratio.max()) if ratio.size else 0.0


def check(b, after):
    """Both parts of the check on the arena after the call; returns the worst error / bound ratio seen."""
    c = b.case
    A, B, C, Ct, P = b.idx
    splits, raw = c["splits"], c["splits"] > 1 and not c["ordered"]
    bits = after.view(np.uint64)
    stray = np.flatnonzero((bits != b.before) & ~b.written)
    assert stray.size == 0, "elements outside the write set changed, first at %s" % stray[:8]
    top = 0.0
    for z in range(c["batch"]):
        if not raw:
            r = worst(after[C[z]], expected_c(b, z), bound_c(b, z), b.mask)
            assert r <= 1.0, ("C", z, r)
            top = max(top, r)
        if Ct:
            assert splits <= 1
            want = np.longdouble(c["alpha"]) * b.prod[z]
            r = worst(after[Ct[z]], want, (c["K"] + 5) * U * abs(c["alpha"]) * b.mag[z], b.mask)
            assert r <= 1.0, ("Ct", z, r)
            top = max(top, r)
        if splits > 1:
            total = np.zeros_like(b.prod[z])
            for s in range(splits):
                got = after[P[z][s]]
                r = worst(got, b.part[z][s], (c["K"] + 4) * U * b.part_mag[z][s], b.mask)
                assert r <= 1.0, ("partial", z, s, r)
                k0, k1 = split_ranges(c["K"], splits)[s]
                if k0 == k1:  # an empty split's partial is zeros, not poison and not what was there
                    assert (got[b.mask] == 0.0).all(), ("empty split", z, s)
                total = total + np.where(b.mask, got, 0.0).astype(np.longdouble)
            if raw:  # the caller's own reduction: summed here in longdouble, held to the same bound
                r = worst(total, b.prod[z], (c["K"] + splits + 4) * U * b.mag[z], b.mask)
                assert r <= 1.0, ("sum of partials", z, r)
                top = max(top, r)
    return top


def logical(b, after, z=0):
    """C of batch member z as an M x N array (for the bit comparisons between layouts)"""
    return after[b.idx[2][z]]


# ------------------------------------------------------------------------------------------------------------------
# The layouts the library's call sites state.  Each returns (case, arena_len); `site` names the file and lines.
# ------------------------------------------------------------------------------------------------------------------
def panel_syrk(ns, k0, nb):
    """kernels_kkt_big.hip.h:458-461  g1 = BigGemm(below, below, nb, L21, ns, L21, ns, D + (k0+nb) + (k0+nb) ns, ns,
    -1, 1, lower_only = 1), LaunchGemm(g1, false, true, 1): A and B are ONE pointer, C a later block of the same D."""
    below = ns - k0 - nb
    ar = Arena()
    D = ar.take(ns * ns, odd=False)
    l21 = D + (k0 + nb) + k0 * ns
    return case(M=below, N=below, K=nb, ta=0, tb=1, offA=l21, lda=ns, offB=l21, ldb=ns,
                offC=D + (k0 + nb) + (k0 + nb) * ns, ldc=ns, alpha=-1.0, beta=1.0, lower_only=1,
                site="kernels_kkt_big.hip.h:458-461"), ar.total()


def panel_gemm(ns, s, k0, nb):
    """kernels_kkt_big.hip.h:463-464  g2 = BigGemm(below, s, nb, L21, ns, B + k0, ns, B + k0 + nb, ns, -1, 1, 0),
    LaunchGemm(g2, false, false, 1): reads rows k0 .. k0 + nb of the off block, writes the rows below them."""
    below = ns - k0 - nb
    ar = Arena()
    D = ar.take(ns * ns)
    Bo = ar.take(ns * s)
    return case(M=below, N=s, K=nb, offA=D + (k0 + nb) + k0 * ns, lda=ns, offB=Bo + k0, ldb=ns,
                offC=Bo + k0 + nb, ldc=ns, alpha=-1.0, beta=1.0, site="kernels_kkt_big.hip.h:463-464"), ar.total()


def separator_update(ns, s):
    """kernels_kkt_big.hip.h:473-474  BigGemm(s, s, ns, B, ns, B, ns, U, s, 1, 0, 0), LaunchGemm(g, true, false, 1)"""
    ar = Arena()
    Bo = ar.take(ns * s)
    Uo = ar.take(s * s + s)
    return case(M=s, N=s, K=ns, ta=1, offA=Bo, lda=ns, offB=Bo, ldb=ns, offC=Uo, ldc=s,
                site="kernels_kkt_big.hip.h:473-474"), ar.total()


def separator_rhs(ns, s):
    """kernels_kkt_big.hip.h:477-478  BigGemm(s, 1, ns, B, ns, b, ns, t, s, 1, 0, 0), LaunchGemm(g, true, false, 1):
    t = ws + s s behind U"""
    ar = Arena()
    Bo = ar.take(ns * s)
    bo = ar.take(ns)
    Uo = ar.take(s * s + s)
    return case(M=s, N=1, K=ns, ta=1, offA=Bo, lda=ns, offB=bo, ldb=ns, offC=Uo + s * s, ldc=s,
                site="kernels_kkt_big.hip.h:477-478"), ar.total()


def lmi_wide(n, m1, count):
    """kernels_lmi_large.hip.h:822-844  M = n, N = n m1, K = n; A = W (lda n, sA1 nn); B = [A_1 .. A_m C] (ldb n,
    sB1 = a_stride); C = PT (ldc n, sC1 m1 nn); Ct = P (ldct n, sT1 m1 nn, ctb n, sTb nn - n); LaunchGemm(a, false,
    false, count)"""
    nn = n * n
    ar = Arena()
    W = ar.take(count * nn)
    Ao = ar.take(count * m1 * nn)
    PT = ar.take(count * m1 * nn)
    Po = ar.take(count * m1 * nn)
    c = case(M=n, N=n * m1, K=n, batch=count, offA=W, lda=n, sA1=nn, offB=Ao, ldb=n, sB1=m1 * nn, offC=PT, ldc=n,
             sC1=m1 * nn, offCt=Po, ldct=n, sT1=m1 * nn, ctb=n, sTb=nn - n, site="kernels_lmi_large.hip.h:822-844")
    ar.cover_ct(c)
    return c, ar.total()


def lmi_folded(n0, d, m1, count):
    """kernels_lmi_large.hip.h:760-782  n = d n0, per = n0 n, stride = m1 nn: M = n, N = n0 m1, K = n; A = W (lda n,
    sA1 nn); B = Aleft (ldb n, sB1 per m1); C = PTl (ldc n, sC1 stride); Ct = P (ldct n0, sT1 stride, ctb n0,
    sTb per - n0); LaunchGemm(a, false, false, count)"""
    n = d * n0
    nn, per = n * n, n0 * n
    stride = m1 * nn
    ar = Arena()
    W = ar.take(count * nn)
    Al = ar.take(count * per * m1)
    PT = ar.take(count * stride)
    Po = ar.take(count * stride)
    c = case(M=n, N=n0 * m1, K=n, batch=count, offA=W, lda=n, sA1=nn, offB=Al, ldb=n, sB1=per * m1, offC=PT, ldc=n,
             sC1=stride, offCt=Po, ldct=n0, sT1=stride, ctb=n0, sTb=per - n0, site="kernels_lmi_large.hip.h:760-782")
    ar.cover_ct(c)
    return c, ar.total()


def lmi_gram(K, m1, count, splits):
    """kernels_lmi_large.hip.h:847-867 (K = nn, lda = ldb = nn, sA1 = sB1 = m1 nn) and :788-807 (K = per = n0 n,
    lda = ldb = per, sA1 = sB1 = stride = m1 nn): M = N = m1; C = Gf (ldc m1, sC1 m1 m1); lower_only; splits with
    sCs = count m1 m1 and C = part: RAW partials through LaunchGemm(a, true, false, count)."""
    stride = m1 * K
    ar = Arena()
    X = ar.take(count * stride)
    Y = ar.take(count * stride)
    Gf = ar.take(count * m1 * m1)
    part = ar.take(splits * count * m1 * m1) if splits > 1 else -1
    return case(M=m1, N=m1, K=K, ta=1, batch=count, offA=X, lda=K, sA1=stride, offB=Y, ldb=K, sB1=stride, offC=Gf,
                ldc=m1, sC1=m1 * m1, lower_only=1, splits=splits, ordered=0, offPart=part, sCs=count * m1 * m1,
                site="kernels_lmi_large.hip.h:847-867"), ar.total()


def lmi_aug(n, count):
    """kernels_lmi_large.hip.h:950-951  SquareGemm(n, aug + nn, 2 nn, W, nn, EW, nn), LaunchGemm(c, false, false,
    count): the right half of the augmented system, batch stride 2 nn"""
    nn = n * n
    ar = Arena()
    aug = ar.take(count * 2 * nn)
    W = ar.take(count * nn)
    EW = ar.take(count * nn)
    return case(M=n, N=n, K=n, batch=count, offA=aug + nn, lda=n, sA1=2 * nn, offB=W, ldb=n, sB1=nn, offC=EW, ldc=n,
                sC1=nn, site="kernels_lmi_large.hip.h:950-951"), ar.total()


def quad_qa1(n, m, count):
    """cone_quad.hip:183-196  T = Q A1: M = n, N = m, K = n; A = Q (lda n, sA1 nn); B = A + 1 (ldb len = n + 1,
    sB1 len m); C = T (ldc n, sC1 n m); LaunchGemm(a, false, false, nb)"""
    ln = n + 1
    ar = Arena()
    Q = ar.take(count * n * n)
    Ao = ar.take(count * ln * m)
    T = ar.take(count * n * m)
    return case(M=n, N=m, K=n, batch=count, offA=Q, lda=n, sA1=n * n, offB=Ao + 1, ldb=ln, sB1=ln * m, offC=T, ldc=n,
                sC1=n * m, site="cone_quad.hip:183-196"), ar.total()


def quad_gram(n, m, count, has_q):
    """cone_quad.hip:199-210  A_gram = A1' T (or A1' A1): M = N = m, K = n; A = A + 1 (lda len, sA1 len m); B = T
    (ldb n, sB1 n m) or A1 again; C = Gram (ldc m, sC1 m m); LaunchGemm(a, true, false, nb)"""
    ln = n + 1
    ar = Arena()
    Ao = ar.take(count * ln * m)
    T = ar.take(count * n * m)
    G = ar.take(count * m * m)
    return case(M=m, N=m, K=n, ta=1, batch=count, offA=Ao + 1, lda=ln, sA1=ln * m,
                offB=T if has_q else Ao + 1, ldb=n if has_q else ln, sB1=n * m if has_q else ln * m,
                offC=G, ldc=m, sC1=m * m, site="cone_quad.hip:199-210"), ar.total()


def factored_slack(n, dR, count, d=1):
    """kernels_lmi_factored.hip.h:258-274  M = n, N = n (d = 1, beta = 1 into S) or n / d (d > 1, beta = 0 into T,
    sC1 = n (n / d)), K = d R; A = Fs, B = F (lda = ldb = n, sA1 = sB1 = nf = n d R); ldc n; LaunchGemm(a, false,
    true, count)"""
    nf = n * dR
    ar = Arena()
    Fs = ar.take(count * nf)
    F = ar.take(count * nf)
    N = n // d
    S = ar.take(count * n * N)
    return case(M=n, N=N, K=dR, tb=1, batch=count, offA=Fs, lda=n, sA1=nf, offB=F, ldb=n, sB1=nf, offC=S, ldc=n,
                sC1=n * N, beta=1.0 if d == 1 else 0.0, site="kernels_lmi_factored.hip.h:258-274"), ar.total()


def gram_lower(ln, m, count, splits, alpha=1.0):
    """cone_linear.hip:146-166  LaunchGramLower: M = N = m, K = len; A = B = WA (lda = ldb = len, sA1 = sB1 = len m);
    C = Gf (ldc m, sC1 m m); alpha; lower_only; splits with sCs = cnt m m; LaunchGemmSplitK(a, true, false, nb, part)"""
    ar = Arena()
    stride = ln * m
    WA = ar.take(count * stride)
    Gf = ar.take(count * m * m)
    part = ar.take(splits * count * m * m) if splits > 1 else -1
    return case(M=m, N=m, K=ln, ta=1, batch=count, offA=WA, lda=ln, sA1=stride, offB=WA, ldb=ln, sB1=stride, offC=Gf,
                ldc=m, sC1=m * m, alpha=alpha, lower_only=1, splits=splits, ordered=1, offPart=part, sCs=count * m * m,
                site="cone_linear.hip:146-166"), ar.total()


def plain(M, N, K, ta, tb, pad=0, batch=1, inner=1, odd=False, **kw):
    """One product on operands of its own: ld = rows + pad (pad = "even": rows + 2 or rows + 3, whichever is even),
    batch members a gap apart, optionally 8 bytes off alignment."""
    ra, ca = (K, M) if ta else (M, K)
    rb, cb = (N, K) if tb else (K, N)
    if pad == "even":
        lda, ldb, ldc, pad = ra + 2 + (ra & 1), rb + 2 + (rb & 1), M + 3, 3
    else:
        lda, ldb, ldc = ra + pad, rb + pad, M + pad
    gap = 2 * (1 + pad)
    sa, sb, sc = lda * ca + gap, ldb * cb + gap, ldc * N + gap
    outer = (batch + inner - 1) // inner
    ar = Arena()
    Ao = ar.take(batch * sa, odd=odd)
    Bo = ar.take(batch * sb, odd=odd)
    Co = ar.take(batch * sc)
    c = case(M=M, N=N, K=K, ta=int(ta), tb=int(tb), batch=batch, inner=inner, offA=Ao, lda=lda, offB=Bo, ldb=ldb,
             offC=Co, ldc=ldc)
    if inner > 1:
        c.update(sA2=sa, sA1=inner * sa, sB2=sb, sB1=inner * sb, sC2=sc, sC1=inner * sc)
    else:
        c.update(sA1=sa, sB1=sb, sC1=sc)
    assert outer * inner == batch
    if kw.get("ct"):
        ldct = N + pad
        st = ldct * M + gap
        To = ar.take(batch * st)
        c.update(offCt=To, ldct=ldct)
        c.update(dict(sT2=st, sT1=inner * st) if inner > 1 else dict(sT1=st))
        ar.cover_ct(c)
    splits = kw.get("splits", 1)
    if splits > 1:
        c.update(splits=splits, ordered=kw.get("ordered", 1), offPart=ar.take(splits * batch * sc), sCs=batch * sc)
    for k in ("alpha", "beta", "lower_only", "tile", "general"):
        if k in kw:
            c[k] = kw[k]
    return c, ar.total()


def fields_of(c):
    """the dict cxk_gemm_f64_layout takes (without alpha, beta and the citation)"""
    return {k: v for k, v in c.items() if k not in ("alpha", "beta", "site")}
