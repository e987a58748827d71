"""Hermitian matrix inequalities given by their entries (cxk_add_hermitian_coo): a generator of cases with the lists and
the dense planes of the same data, the embedding the library documents (block (k, j) of L(X) is sign[k ^ j][j] X_{k ^ j}
at row k n + r, column j n + c), a numpy model of the folded sums (kernels_lmi_sparse.hip.h: the first list of every sum
runs over its top block row, no 1 / d), the dense formulas it is compared with, and the refusal table.  No GPU."""
import numpy as np

from conex_amd.synthetic import HC_SIGN

SEED = 20260611


def make_case(n, d, m, per=2, seed=SEED, c="identity", c_diag=None, full_a=False, empty_a=None, off_planes=None,
              diag_only=False):
    """One constraint of order n over R / C / H (d planes) in m variables.  A_i has `per` lower-triangle entries (an int,
    or one per matrix), the first on the diagonal, at a position that differs between the first n matrices (all of the
    lower triangle with full_a; the diagonal alone with diag_only).  Diagonal entries lie in [1, 2], off-diagonal planes
    in +-[0.3, 1], so that no tested sum is the small difference of large terms: a relative bar then measures the
    summation, not the data's cancellation.  A_{empty_a} is the zero matrix.  off_planes: the planes an off-diagonal
    entry uses (default all; (1,) purely imaginary for d = 2, (3,) the last plane alone for d = 4).
    C: "identity", "full" (Hermitian, diagonally dominant) or, with c_diag = k, the first k diagonal ones (not
    definite: assembly only).  Returns the lists (shuffled within a list, val (nnz, d)) and the planes A (m, d, n, n),
    C (d, n, n)."""
    rng = np.random.default_rng(seed + 1000 * n + 10 * m + d)
    planes = tuple(range(d)) if off_planes is None else tuple(off_planes)

    def value(r, c_):
        v = np.zeros(d)
        if r == c_:
            v[0] = rng.uniform(1.0, 2.0)
        for p in (() if r == c_ else planes):
            v[p] = rng.uniform(0.3, 1.0) * rng.choice([-1.0, 1.0])
        return v

    lists = []
    pers = [per] * m if np.isscalar(per) else list(per)
    first = rng.permutation(n)
    for i in range(m):
        per = pers[i]
        if i == empty_a:
            lists.append({})
            continue
        if full_a:
            pos = [(r, c_) for c_ in range(n) for r in range(c_, n)]
        elif diag_only:
            pos = [(int(k), int(k)) for k in rng.choice(n, size=min(per, n), replace=False)]
        else:
            k = int(first[i % n])
            pos = {(k, k)}
            while len(pos) < min(per, n * (n + 1) // 2):
                a, b = (int(t) for t in rng.integers(n, size=2))
                pos.add((max(a, b), min(a, b)))
            pos = sorted(pos)
        lists.append({p: value(*p) for p in pos})
    if c_diag is not None:
        lists.append({(k, k): np.r_[1.0, np.zeros(d - 1)] for k in range(c_diag)})
    elif c == "full":
        ent = {(r, c_): 0.3 * value(r, c_) for c_ in range(n) for r in range(c_, n)}
        for k in range(n):
            ent[(k, k)] = np.r_[2.0 + 0.3 * d * n, np.zeros(d - 1)]
        lists.append(ent)
    else:
        lists.append({(k, k): np.r_[1.0, np.zeros(d - 1)] for k in range(n)})
    ptr, row, col, val = [0], [], [], []
    M = np.zeros((m + 1, d, n, n))
    for i, ent in enumerate(lists):
        keys = sorted(ent)
        for q in rng.permutation(len(keys)):
            r, c_ = keys[q]
            v = ent[keys[q]]
            row.append(r), col.append(c_), val.append(v)
            M[i, :, r, c_] = v
            if r != c_:
                M[i, 0, c_, r] = v[0]
                M[i, 1:, c_, r] = -v[1:]
        ptr.append(len(row))
    return dict(n=n, d=d, m=m, ptr=np.array(ptr, np.int32), row=np.array(row, np.int32), col=np.array(col, np.int32),
                val=np.array(val, np.float64).reshape(-1, d), A=M[:m], C=M[m])


def embed_planes(X):
    """L(X) of planes X (d, n, k): block (k, j) = sign[k ^ j][j] X_{k ^ j}."""
    d, n, k = X.shape
    out = np.zeros((d * n, d * k), dtype=X.dtype)
    for a in range(d):
        for j in range(d):
            out[a * n:(a + 1) * n, j * k:(j + 1) * k] = HC_SIGN[a ^ j, j] * X[a ^ j]
    return out


def embedded_list(case, i):
    """The nonzeros of L(matrix i) as (row, col, val), both triangles, sorted by column then row, built from the list
    by the block rule: the device's (unfolded) order."""
    n, d = case["n"], case["d"]
    R, C_, V = [], [], []
    for e in range(case["ptr"][i], case["ptr"][i + 1]):
        r, c_, v = int(case["row"][e]), int(case["col"][e]), case["val"][e]
        for p in range(d):
            if v[p] == 0.0:
                continue
            for j in range(d):
                k = p ^ j
                a = HC_SIGN[p, j] * v[p]
                R.append(k * n + r), C_.append(j * n + c_), V.append(a)
                if r != c_:
                    R.append(k * n + c_), C_.append(j * n + r), V.append(-a if p else a)
    R, C_, V = np.array(R, dtype=np.int64), np.array(C_, dtype=np.int64), np.array(V, dtype=np.float64)
    o = np.lexsort((R, C_))
    return R[o], C_[o], V[o]


def folded_order(case, i):
    """... in the folded order: the top block row (rows below n) first, then the rest, each by column then row; and
    the number of the former."""
    R, C_, V = embedded_list(case, i)
    top = R < case["n"]
    o = np.r_[np.flatnonzero(top), np.flatnonzero(~top)]
    return R[o], C_[o], V[o], int(top.sum())


def folded_model(case, W):
    """G, AW, AQc, <c,Qc>, <w,c> as a folded group forms them with C riding in the pair sums: every sum over a first
    list runs over its top entries, the second list is whole, nothing is divided by d.  Returns also the counts
    (top, all) over the m + 1 lists."""
    m = case["m"]
    L = [folded_order(case, i) for i in range(m + 1)]

    def pair(i, j):
        r, c_, a, t = L[i]
        p, q, b, _ = L[j]
        r, c_, a = r[:t], c_[:t], a[:t]
        return float(a @ ((W[np.ix_(c_, p)] * W[np.ix_(q, r)].T) @ b))

    G = np.array([[pair(i, j) for j in range(m)] for i in range(m)]).reshape(m, m)
    AW = np.array([float(L[i][2][:L[i][3]] @ W[L[i][1][:L[i][3]], L[i][0][:L[i][3]]]) for i in range(m + 1)])
    AQc = np.array([pair(i, m) for i in range(m)])
    return dict(G=G, AW=AW[:m], AQc=AQc, cq=pair(m, m), wc=AW[m], top=sum(l[3] for l in L), all=sum(len(l[0]) for l in L))


def dense_formulas(case, W, dtype=np.longdouble):
    """tr(L(A_i) W L(A_j) W) / d, tr(L(A_i) W) / d, tr(L(A_i) W L(C) W) / d, tr(L(C) W L(C) W) / d, tr(L(C) W) / d on
    the embedded matrices."""
    d, m = case["d"], case["m"]
    A = [embed_planes(a).astype(dtype) for a in case["A"]]
    C_ = embed_planes(case["C"]).astype(dtype)
    W = W.astype(dtype)
    P = [W @ a for a in A]
    PC = W @ C_
    G = np.array([[np.sum(pi * pj.T) for pj in P] for pi in P], dtype=dtype).reshape(m, m) / d
    AW = np.array([np.trace(p) for p in P], dtype=dtype) / d
    AQc = np.array([np.sum(p * PC.T) for p in P], dtype=dtype) / d
    return dict(G=G, AW=AW, AQc=AQc, cq=np.sum(PC * PC.T) / d, wc=np.trace(PC) / d)


def hermitian_exponential(n, d, seed=SEED + 5, scale=0.3):
    """W = L(exp(H)) for a random Hermitian H: the real representation of a Hermitian positive definite matrix, formed as
    the library forms the W it is given (cxk_set_W takes planes and embeds them): the planes of exp(L(H)) re-embedded,
    so that the block structure is exact."""
    rng = np.random.default_rng(seed + n + d)
    R = rng.standard_normal((d, n, n))
    H = np.empty_like(R)
    H[0] = R[0] + R[0].T
    for p in range(1, d):
        H[p] = R[p] - R[p].T
    S = embed_planes(H) * (scale / np.sqrt(d * n))
    assert np.array_equal(S, S.T)
    lam, Q = np.linalg.eigh(S)
    E = (Q * np.exp(lam)) @ Q.T
    planes = np.stack([E[k * n:(k + 1) * n, :n] for k in range(d)])  # block (k, 0) = X_k
    planes[0] = 0.5 * (planes[0] + planes[0].T)
    for k in range(1, d):
        planes[k] = 0.5 * (planes[k] - planes[k].T)
    return embed_planes(planes)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


MODEL_SHAPES = [(n, d, m) for d in (2, 4) for (n, m) in ((4, 1), (9, 3), (33, 5))]

# cxk_add_hermitian_coo's refusals: (n, d, m, ptr, row, col, val (d per entry), message after "cxk_add_hermitian_coo: ")
R_PACK = ("d n or m is above 32767 (the entry table packs row | col << 16 and the pair table i | j << 16 into ints that "
          "the kernels unpack with signed shifts)")
R_DIAGONAL = "a diagonal entry has a nonzero plane beyond the first (the diagonal of a Hermitian matrix is real)"
R_OCTONIONS = "hyper-complex dimension 8: the octonions have no real representation, entries are for d = 1, 2, 4"
NAN = float("nan")
REFUSALS = [
    (0, 2, 1, [0, 0, 0], [], [], [], "n is at least 1 and m at least 0"),
    (4, 2, -1, [0, 0], [], [], [], "n is at least 1 and m at least 0"),
    (4, 8, 1, [0, 0, 0], [], [], [], R_OCTONIONS),
    (4, 3, 1, [0, 0, 0], [], [], [], "the hyper-complex dimension is 1, 2 or 4"),
    (4, 0, 1, [0, 0, 0], [], [], [], "the hyper-complex dimension is 1, 2 or 4"),
    (4, 2, 1, [1, 1, 1], [0], [0], [1.0, 0.0], "ptr[0] is not 0"),
    (4, 2, 1, [0, 2, 1], [0, 1], [0, 1], [1.0, 0.0, 1.0, 0.0], "ptr decreases"),
    (4, 2, 1, [0, 1, 2], [0, 4], [0, 0], [1.0, 0.0, 1.0, 0.0], "an index is outside [0, n)"),
    (4, 2, 1, [0, 1, 2], [0, 1], [0, -1], [1.0, 0.0, 1.0, 0.0], "an index is outside [0, n)"),
    (4, 2, 1, [0, 1, 2], [0, 1], [0, 2], [1.0, 0.0, 1.0, 0.5],
     "an entry lies above the diagonal (row < col): the lower triangle is given"),
    (4, 2, 1, [0, 2, 3], [2, 2, 1], [1, 1, 1], [1.0, 0.5, 2.0, 0.0, 1.0, 0.0], "a list names a position twice"),
    (4, 2, 1, [0, 2, 3], [2, 2, 1], [1, 1, 1], [0.0, 0.0, 2.0, 0.0, 1.0, 0.0], "a list names a position twice"),
    (4, 2, 1, [0, 1, 2], [0, 1], [0, 1], [1.0, 0.0, 1.0, NAN], "a value is not finite"),
    (4, 4, 1, [0, 1, 2], [0, 1], [0, 0], [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, float("inf"), 0.0], "a value is not finite"),
    (4, 2, 1, [0, 1, 2], [0, 1], [0, 1], [1.0, 0.0, 1.0, 0.25], R_DIAGONAL),
    (4, 4, 1, [0, 1, 2], [0, 1], [0, 1], [1.0, 0.0, 0.0, -1.0, 1.0, 0.0, 0.0, 0.0], R_DIAGONAL),
    (16384, 2, 1, [0, 0, 0], [], [], [], R_PACK),
    (8192, 4, 1, [0, 0, 0], [], [], [], R_PACK),
]
R_FINALIZE = ("a matrix inequality added by cxk_add_hermitian_coo has no dense matrices and can only take the sparse "
              "route (CXK_SPARSE_LMI, which is 0)")
