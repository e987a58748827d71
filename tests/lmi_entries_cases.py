"""Matrix inequalities given by their entries (cxk_add_lmi_coo): a generator of cases with the lists and the dense
matrices of the same data, a numpy model of the restricted evaluation of the affine term (W C W formed only where an
entry reads it: kernels_lmi_sparse.hip.h, lmi_affine_*), and the dense formulas it is compared with.  No GPU."""
import numpy as np

SEED = 20260417


def _lower_positions(rng, n, count, diag, exclude=()):
    """`count` distinct positions of the lower triangle, `diag` of them on the diagonal, none touching `exclude`."""
    idx = np.array([i for i in range(n) if i not in set(exclude)])
    d = rng.choice(idx, size=diag, replace=False)
    pos = {(int(i), int(i)) for i in d}
    while len(pos) < count:
        i, j = (int(t) for t in rng.choice(idx, size=2, replace=False))
        pos.add((max(i, j), min(i, j)))
    return sorted(pos)


def make_case(n, m, nnz_c, seed=SEED, diag_only=False, empty_index=None, empty_a=None, a_entries=3):
    """One constraint of order n over m variables.  C has exactly nnz_c nonzeros counting both triangles (all on the
    diagonal with diag_only); row and column `empty_index` of C hold nothing; A_i has `a_entries` lower-triangle entries,
    the first on C's pattern where C has an off-diagonal entry, one on the diagonal, the rest anywhere (so on and off C's
    pattern); A_{empty_a} is the zero matrix.  Returns the lists (lower triangles, shuffled within a list), and the
    dense A (m, n, n) and C (n, n) of the same data."""
    rng = np.random.default_rng(seed + 1000 * n + 10 * m + nnz_c)
    excl = () if empty_index is None else (empty_index,)
    if diag_only:
        assert nnz_c <= n - len(excl)
        cpos = _lower_positions(rng, n, nnz_c, nnz_c, excl)
    else:
        diag = nnz_c % 2 + 2 * min(2, (n - len(excl) - nnz_c % 2) // 2)  # parity of nnz_c, plus a few
        diag = min(diag, nnz_c)
        if (nnz_c - diag) % 2:
            diag -= 1
        cpos = _lower_positions(rng, n, diag + (nnz_c - diag) // 2, diag, excl)
    lists = []
    for i in range(m):
        if i == empty_a:
            lists.append([])
            continue
        pos = set()
        off = [p for p in cpos if p[0] != p[1]]
        if off:
            pos.add(off[int(rng.integers(len(off)))])
        k = int(rng.integers(n))
        pos.add((k, k))
        while len(pos) < a_entries:
            a, b = (int(t) for t in rng.integers(n, size=2))
            pos.add((max(a, b), min(a, b)))
        lists.append(sorted(pos))
    lists.append(cpos)
    ptr, row, col, val = [0], [], [], []
    A = np.zeros((m, n, n))
    C = np.zeros((n, n))
    for i, pos in enumerate(lists):
        order = rng.permutation(len(pos))
        for k in order:
            r, c = pos[k]
            v = float(rng.uniform(0.3, 1.0) * rng.choice([-1.0, 1.0]))
            if i == m and r == c:
                v = abs(v) + 1.0  # (a strictly feasible start y = 0 needs C positive definite on its support)
            row.append(r), col.append(c), val.append(v)
            M = A[i] if i < m else C
            M[r, c] = M[c, r] = v
        ptr.append(len(row))
    assert np.count_nonzero(C) == nnz_c, (np.count_nonzero(C), nnz_c)
    return dict(n=n, m=m, ptr=np.array(ptr, np.int32), row=np.array(row, np.int32), col=np.array(col, np.int32),
                val=np.array(val, np.float64), A=A, C=C)


def symmetric_w(n, seed=SEED + 5, scale=0.3):
    """A symmetric positive definite W != I (the scaling point of synthetic.scaling_points, one member)."""
    rng = np.random.default_rng(seed + n)
    S = rng.standard_normal((n, n))
    S = 0.5 * (S + S.T) * scale / np.sqrt(n)
    lam, Q = np.linalg.eigh(S)
    W = (Q * np.exp(lam)) @ Q.T
    return 0.5 * (W + W.T)


def mirrored(case, i):
    """Both triangles of list i as (row, col, val), sorted by column then row: the device's order."""
    s = slice(case["ptr"][i], case["ptr"][i + 1])
    r, c, v = case["row"][s], case["col"][s], case["val"][s]
    off = r != c
    rr, cc, vv = np.r_[r, c[off]], np.r_[c, r[off]], np.r_[v, v[off]]
    keep = vv != 0.0
    rr, cc, vv = rr[keep], cc[keep], vv[keep]
    o = np.lexsort((rr, cc))
    return rr[o], cc[o], vv[o]


def restricted_model(case, W):
    """AQc, <c,Qc>, <w,c> as the device forms them: U = (W C)' from C's columns, X = W C W only at the positions P
    that an entry of some A_i or of C names, then the sums over the entries.  Returns (AQc, cq, wc, |P|)."""
    n, m = case["n"], case["m"]
    cr, cc, cv = mirrored(case, m)
    U = np.zeros((n, n))          # U[p, c] = sum_{q in column p of C} C[q, p] W[c, q]
    for q, p, v in zip(cr, cc, cv):
        U[p, :] += v * W[:, q]
    lists = [mirrored(case, i) for i in range(m)]
    P = sorted({(int(c), int(r)) for (rr, cc_, _) in lists + [(cr, cc, cv)] for r, c in zip(rr, cc_)})
    X = {(c, r): float(U[:, c] @ W[:, r]) for (c, r) in P}  # X[c, r] = sum_p U[p, c] W[p, r]
    AQc = np.array([sum(a * X[(int(c), int(r))] for r, c, a in zip(*L)) for L in lists])
    cq = sum(v * X[(int(p), int(q))] for q, p, v in zip(cr, cc, cv))
    wc = sum(v * W[p, q] for q, p, v in zip(cr, cc, cv))
    return AQc, cq, wc, len(P)


def dense_formulas(case, W, dtype=np.longdouble):
    """X = W C W, AQc(i) = tr(A_i X), <c,Qc> = tr(C X), <w,c> = tr(C W), G(i,j) = tr(W A_i W A_j), AW(i) = tr(A_i W)."""
    A, C, W = case["A"].astype(dtype), case["C"].astype(dtype), W.astype(dtype)
    X = W @ C @ W
    AQc = np.array([np.sum(Ai * X.T) for Ai in A], dtype=dtype)
    P = [W @ Ai for Ai in A]
    G = np.array([[np.sum(Pi * Pj.T) for Pj in P] for Pi in P], dtype=dtype).reshape(len(A), len(A))
    AW = np.array([np.sum(Ai * W.T) for Ai in A], dtype=dtype)
    return dict(AQc=AQc, cq=np.sum(C * X.T), wc=np.sum(C * W.T), G=G, AW=AW)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


# (n, m, nnz C) of the issue's scratch run; the restricted form was within 1.4e-15 of longdouble there
MODEL_SHAPES = [(64, 1, 65), (65, 3, 65), (130, 7, 400), (257, 5, 2000)]

# cxk_add_lmi_coo's refusals: (n, m, ptr, row, col, val, message after "cxk_add_lmi_coo: ")
R_PACK = ("n or m is above 32767 (the entry table packs row | col << 16 and the pair table i | j << 16 into ints that "
          "the kernels unpack with signed shifts)")
REFUSALS = [
    (0, 1, [0, 0, 0], [], [], [], "n is at least 1 and m at least 0"),
    (4, -1, [0, 0], [], [], [], "n is at least 1 and m at least 0"),
    (4, 1, [1, 1, 1], [0], [0], [1.0], "ptr[0] is not 0"),
    (4, 1, [0, 2, 1], [0, 1], [0, 1], [1.0, 1.0], "ptr decreases"),
    (4, 1, [0, 1, 2], [0, 4], [0, 0], [1.0, 1.0], "an index is outside [0, n)"),
    (4, 1, [0, 1, 2], [0, 1], [0, -1], [1.0, 1.0], "an index is outside [0, n)"),
    (4, 1, [0, 1, 2], [0, 1], [0, 2], [1.0, 1.0], "an entry lies above the diagonal (row < col): the lower triangle is given"),
    (4, 1, [0, 2, 3], [2, 2, 1], [1, 1, 1], [1.0, 2.0, 1.0], "a list names a position twice"),
    (4, 1, [0, 1, 2], [0, 1], [0, 1], [1.0, float("nan")], "a value is not finite"),
    (4, 1, [0, 1, 2], [0, 1], [0, 1], [float("inf"), 1.0], "a value is not finite"),
    (32768, 1, [0, 0, 0], [], [], [], R_PACK),
]
R_FINALIZE = ("a matrix inequality added by cxk_add_lmi_coo has no dense matrices and can only take the sparse route "
              "(CXK_SPARSE_LMI, which is 0)")
