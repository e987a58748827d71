"""Quadratic cones whose (n + 1) x m matrix A is given by its nonzeros (cxk_add_quadratic_csr): the rows of
test_gpu_quad_sparse.py / test_quad_sparse_reference.py, their data, the reference restated for a CSR A, and the
context class that lets test_gpu_cone_kernel_matrix.run_rows / build serve unchanged.  numpy only.

Data.  A cone is the dict km.make_cone makes for kind "quad": cn["A"] is the dense (n + 1) x m array whose zeros are
the pattern (the reference and the oracle read it as it is), cn["Q"] is None, a dense array, or the expansion of parts
(quad_structured_cases.ExpandedQ; cn["parts"] holds them).  SparseAQuad.add_quadratic hands the nonzeros of cn["A"] to
add_quadratic_csr, and the parts behind an ExpandedQ with them; the device never sees the dense A.

Signs.  S, F and sigma of the structured rows are nonnegative, as in quad_structured_cases.py, so that the magnitudes
the reference derives from |Q| are those of the evaluation by parts.  A is signed: its zeros carry zero magnitude, so
an entry of G that the pattern makes zero has to come out exactly zero.

Every row is the smallest shape at which its edge exists; test_rows_sit_on_their_edges recomputes each edge with the
launch site's arithmetic.
"""
import numpy as np

import cone_reference as ref
import quad_structured_cases as qc
from conex_amd import KktContext
from conex_amd import synthetic as syn

LD = ref.LD

WAVE = 64               # lanes of the wavefront that strides over a column (quad_sparse_columns / _gather / _scatter)
SLACK_ROW_TILE = 256    # kSocStreamRowTile: rows per workgroup of soc_sparse_slack
BLOCK = 256             # kQuadStreamBlock: entries of G per workgroup of quad_stream_schur_finish
PANEL_BYTES = 256 << 20  # kQuadGramPanelBytes (cone_route.h)
PANEL_MIN, PANEL_MAX = 4, 64  # kQuadGramPanelMinCols, kQuadGramPanelMaxCols


def panel_cols(n, count):
    """QuadGramPanelCols (cone_route.h), restated."""
    return int(min(PANEL_MAX, max(PANEL_MIN, PANEL_BYTES // (2 * 8 * max(count, 1) * max(n, 1)))))


# (id, K, n, m, Q form, pattern of A); a Q form is None (the identity), "dense", or (kind of S or None, rank)
ROWS = [
    ("min", 1, 1, 1, None, "full"),                                   # smallest
    ("selection", 1, 40, 41, "dense", "selection"),                   # the portfolio shape: one-entry columns
    ("empty", 1, 20, 4, ("diagonal", 0), "empty"),                    # empty extents in CSR and CSC
    ("long-column", 1, 300, 3, ("tridiagonal", 2), "long-column"),    # more than four strides of 64 lanes
    ("row-tile", 1, 257, 3, ("tridiagonal", 3), "full"),              # second 256-row tile of the slack; short step
    ("panel", 2, 64, panel_cols(64, 2) + 1, "dense", "two-per-column"),  # last Gram panel of one column
    ("group-of-3", 3, 300, 5, ("bands", 4), "per-row-1-2-all"),       # one group, different nnz, eptr
    ("full-none", 1, 33, 6, None, "full"),                            # the sparse kernels on dense data ...
    ("full-dense", 1, 33, 6, "dense", "full"),
    ("full-parts", 1, 33, 6, ("tridiagonal", 2), "full"),             # ... under each form of Q
]
ROW_IDS = [r[0] for r in ROWS]
SHORT_STEP_ROWS = ("row-tile",)


# ------------------------------------------------------------------------------------ patterns
def pattern_matrix(pattern, n, m, member, rng):
    """The dense (n + 1) x m array of a pattern: its zeros are the pattern."""
    A = rng.uniform(-1, 1, (n + 1, m))
    A[A == 0] = 0.5
    if pattern == "full":
        return A
    if pattern == "selection":  # A1 = [I 0], A0 = e_m
        assert m == n + 1
        S = np.zeros((n + 1, m))
        S[1 + np.arange(n), np.arange(n)] = 1.0
        S[0, m - 1] = 1.0
        return S
    if pattern == "empty":  # row 0, rows 3, 7, 11 of A1 and column 2 without a nonzero
        A[0] = 0.0
        A[1 + np.array([3, 7, 11])] = 0.0
        A[:, 2] = 0.0
        return A
    if pattern == "long-column":  # column 0 full (row 0 included), one entry in every other column
        keep = np.zeros_like(A, dtype=bool)
        keep[:, 0] = True
        keep[1 + rng.integers(0, n, m - 1), np.arange(1, m)] = True
        return np.where(keep, A, 0.0)
    if pattern == "two-per-column":
        keep = np.zeros_like(A, dtype=bool)
        for j in range(m):
            keep[rng.choice(n + 1, 2, replace=False), j] = True
        return np.where(keep, A, 0.0)
    if pattern == "per-row-1-2-all":  # members with 1 / 2 / all entries per row
        per = (1, 2, m)[member]
        keep = np.zeros_like(A, dtype=bool)
        for r in range(n + 1):
            keep[r, rng.choice(m, per, replace=False)] = True
        return np.where(keep, A, 0.0)
    raise ValueError(pattern)


def csr_of(A):
    """(indptr, indices, data) of the nonzeros of the dense (n + 1) x m array, columns ascending."""
    return qc.csr_from_dense(A)


def descending(csr):
    """The same nonzeros with the columns of every row in descending order."""
    indptr, indices, data = csr
    idx, val = indices.copy(), data.copy()
    for r in range(len(indptr) - 1):
        idx[indptr[r]:indptr[r + 1]] = indices[indptr[r]:indptr[r + 1]][::-1]
        val[indptr[r]:indptr[r + 1]] = data[indptr[r]:indptr[r + 1]][::-1]
    return indptr, idx, val


# ------------------------------------------------------------------------------------ the reference for a CSR A
def _pairs(ptr, keys):
    """For every position p of `keys` and every entry e of list keys[p] (ptr[k] <= e < ptr[k + 1]): (p, e), listed."""
    keys = np.asarray(keys, dtype=np.int64)
    ptr = np.asarray(ptr, dtype=np.int64)
    cnt = ptr[keys + 1] - ptr[keys]
    src = np.repeat(np.arange(len(keys)), cnt)
    first = np.repeat(ptr[keys], cnt)
    within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return src, first + within


class Rows1:
    """A1 (rows 1 .. n of a CSR matrix of n + 1 rows) by rows and by entries, and A0 as a dense vector."""

    def __init__(self, csr, m):
        indptr, indices, data = (np.asarray(x) for x in csr)
        self.m, self.n = m, len(indptr) - 2
        self.A0 = np.zeros(m, dtype=LD)
        self.A0[indices[:indptr[1]]] = ref.ld(data[:indptr[1]])
        self.ptr = indptr[1:].astype(np.int64) - int(indptr[1])  # rows of A1
        self.col = indices[indptr[1]:].astype(np.int64)
        self.val = ref.ld(data[indptr[1]:])
        self.row = np.repeat(np.arange(self.n), np.diff(self.ptr))

    def t_dot(self, x, absolute=False):
        """A1' x (x dense, n or n x k)."""
        v = np.abs(self.val) if absolute else self.val
        out = np.zeros((self.m,) + x.shape[1:], dtype=LD)
        np.add.at(out, self.col, v[:, None] * x[self.row] if x.ndim == 2 else v * x[self.row])
        return out

    def gram_csr(self, S, absolute):
        """A1' S A1 for S in CSR, through the nonzeros alone: B = S A1 entry by entry, then A1' B."""
        sp, si, sv = (np.asarray(x) for x in S)
        sv = np.abs(ref.ld(sv)) if absolute else ref.ld(sv)
        av = np.abs(self.val) if absolute else self.val
        s_row = np.repeat(np.arange(self.n), np.diff(sp))
        src, e = _pairs(self.ptr, si)                # S entry (r, c) with every entry (c, j) of A1
        b_row, b_col, b_val = s_row[src], self.col[e], sv[src] * av[e]
        src, e = _pairs(self.ptr, b_row)             # B entry (r, j) with every entry (r, i) of A1
        G = np.zeros((self.m, self.m), dtype=LD)
        np.add.at(G, (self.col[e], b_col[src]), av[e] * b_val[src])
        return G


def _identity_csr(n):
    return np.arange(n + 1), np.arange(n), np.ones(n)


def _gram(a, n, Q, parts, absolute):
    if parts is None and Q is not None:  # dense: small orders only
        Qd = np.abs(ref.ld(Q)) if absolute else ref.ld(Q)
        return a.t_dot(Qd @ _dense_a1(a, absolute), absolute)
    S = _identity_csr(n) if parts is None else parts["S"]
    G = np.zeros((a.m, a.m), dtype=LD) if S is None else a.gram_csr(S, absolute)
    if parts is not None and parts["F"] is not None:
        F = ref.ld(parts["F"])
        sg = np.ones(F.shape[1], dtype=LD) if parts["sigma"] is None else ref.ld(parts["sigma"])
        if absolute:
            F, sg = np.abs(F), np.abs(sg)
        P = a.t_dot(F, absolute)  # m x rank
        G = G + (P * sg) @ P.T
    return G


def _dense_a1(a, absolute):
    A1 = np.zeros((a.n, a.m), dtype=LD)
    A1[a.row, a.col] = np.abs(a.val) if absolute else a.val
    return A1


def _apply(Q, parts, x, absolute):
    if parts is not None:
        return qc.apply_abs_q(parts, x) if absolute else qc.apply_q(parts, x)
    if Q is None:
        return ref.ld(x)
    return (np.abs(ref.ld(Q)) if absolute else ref.ld(Q)) @ ref.ld(x)


def quad_schur_op(csr, m, c, W, Q=None, parts=None):
    """cone_reference.quad_schur restated for A given as (indptr, indices, data) of n + 2 pointers and m columns: G,
    AW, AQc and the two scalars, each with its magnitude (g = 1).  Q: `parts` (as quad_structured_cases takes them),
    else the dense Q, else the identity.  Nothing of n x m is formed unless Q is dense."""
    c, W = ref.ld(c), ref.ld(W)
    ac, aW = np.abs(c), np.abs(W)
    a = Rows1(csr, m)
    n = a.n
    A0, a0 = a.A0, np.abs(a.A0)
    qw, qwm = _apply(Q, parts, W[1:], False), _apply(Q, parts, aW[1:], True)
    qcv, qcm = _apply(Q, parts, c[1:], False), _apply(Q, parts, ac[1:], True)
    det, detm = W[0] * W[0] - W[1:] @ qw, W[0] * W[0] + aW[1:] @ qwm
    scale, scalem = qw @ c[1:] + c[0] * W[0], qwm @ ac[1:] + ac[0] * aW[0]
    v, vm = a.t_dot(qw) + A0 * W[0], a.t_dot(qwm, True) + a0 * aW[0]
    gram, gramm = _gram(a, n, Q, parts, False), _gram(a, n, Q, parts, True)
    t, tm = np.outer(A0, A0) - gram, np.outer(a0, a0) + gramm
    G = 2 * (-det * t + 2 * np.outer(v, v))
    Gm = 2 * (ref.mulm(det, detm, t, tm) + 2 * ref.mulm(v[:, None], vm[:, None], v[None, :], vm[None, :]))
    r, rm = a.t_dot(qcv) - A0 * c[0], a.t_dot(qcm, True) + a0 * ac[0]
    AQc = 2 * (det * r + 2 * v * scale)
    AQcm = 2 * (ref.mulm(det, detm, r, rm) + 2 * ref.mulm(v, vm, scale, scalem))
    z, zm = c[1:] @ qcv - c[0] * c[0], ac[1:] @ qcm + c[0] * c[0]
    s1 = 2 * (det * z + 2 * scale * scale)
    s1m = 2 * (ref.mulm(det, detm, z, zm) + 2 * ref.mulm(scale, scalem, scale, scalem))
    return dict(G=(G, Gm), AW=(2 * v, 2 * vm), AQc=(AQc, AQcm), sc=(ref.ld([2 * scale, s1]), ref.ld([2 * scalem, s1m])), g=1.0)


# ------------------------------------------------------------------------------------ problems
def make_cone(n, m, q_form, pattern, member, point, rng):
    """km.make_cone's quadratic cone with the given form of Q and pattern of A."""
    c = 0.2 * rng.uniform(-1, 1, n + 1)
    c[0] = 1.0
    Q, parts = None, None
    if q_form == "dense":
        R = rng.uniform(-1, 1, (n, n))
        Q = R @ R.T / n + np.eye(n) if point == "well" else ref.conditioned_Q(rng, n, 1e6)
    elif q_form is not None:
        parts = qc.make_parts(q_form[0], n, q_form[1], member, rng)
        Q = qc.expand(parts, n)
    A = pattern_matrix(pattern, n, m, member, rng)
    return dict(kind="quad", m=m, A=A, c=c, Q=Q, parts=parts,
                W=ref.spin_scaling_point(rng, n, point, None if Q is None else np.asarray(Q, dtype=np.float64)))


def row_seed(row):
    _, K, n, m, _, _ = row
    return 11000 + 31 * n + 7 * m + K + 5 * ROW_IDS.index(row[0])


def make_problem(row, point, seed=None):
    """(cones, cliques, num_vars): K cones in a chain of cliques, as km.make_problem arranges them."""
    _, K, n, m, q_form, pattern = row
    rng = np.random.default_rng(row_seed(row) if seed is None else seed)
    cliques, num_vars = syn.chain_cliques(K, m, 1 if m > 1 else 0)
    return [make_cone(n, m, q_form, pattern, k, point, rng) for k in range(K)], cliques, num_vars


def q_argument(Q):
    """What add_quadratic_csr takes for a cone's Q: the parts behind an ExpandedQ, else Q itself."""
    parts = getattr(Q, "parts", None)
    return parts if parts is not None else Q


class SparseAQuad(KktContext):
    """A KktContext whose add_quadratic hands the nonzeros of the dense A to add_quadratic_csr (and the parts behind an
    ExpandedQ with them)."""

    order_of_columns = staticmethod(lambda csr: csr)

    def add_quadratic(self, Q, A, c, vars_=None):
        return self.add_quadratic_csr(q_argument(Q), self.order_of_columns(csr_of(A)), c, vars_)


class DescendingSparseAQuad(SparseAQuad):
    """... with the columns of every row handed over in descending order."""

    order_of_columns = staticmethod(descending)


# ------------------------------------------------------------------------------------ the edges
def test_rows_sit_on_their_edges():
    shape = {r[0]: r for r in ROWS}
    mats = {r[0]: [cn["A"] for cn in make_problem(r, "well")[0]] for r in ROWS}
    per_col = {k: [(A != 0).sum(axis=0) for A in v] for k, v in mats.items()}
    per_row = {k: [(A != 0).sum(axis=1) for A in v] for k, v in mats.items()}
    _, K, n, m, q, _ = shape["min"]
    assert (K, n, m, q) == (1, 1, 1, None) and per_col["min"][0][0] == 2
    _, K, n, m, q, _ = shape["selection"]
    A = mats["selection"][0]
    assert m == n + 1 and q == "dense" and np.all(per_col["selection"][0] == 1)
    assert np.array_equal(A[1:, :n], np.eye(n)) and np.all(A[1:, n] == 0) and np.array_equal(A[0], np.eye(m)[m - 1])
    _, K, n, m, q, _ = shape["empty"]
    assert q == ("diagonal", 0) and per_row["empty"][0][0] == 0 and np.sum(per_row["empty"][0][1:] == 0) >= 3
    assert np.sum(per_col["empty"][0] == 0) == 1
    _, K, n, m, q, _ = shape["long-column"]
    cols = per_col["long-column"][0]
    assert cols[0] == n + 1 and cols[0] > 4 * WAVE and np.all(cols[1:] == 1) and q[1] == 2
    _, K, n, m, q, _ = shape["row-tile"]
    assert (n + 1 + SLACK_ROW_TILE - 1) // SLACK_ROW_TILE == 2 and n % SLACK_ROW_TILE == 1 and "row-tile" in SHORT_STEP_ROWS
    assert np.all(per_row["row-tile"][0] == 3) and q[1] == 3
    _, K, n, m, q, _ = shape["panel"]
    P = panel_cols(n, K)
    assert K == 2 and m == P + 1 and (m + P - 1) // P == 2 and m - P == 1  # two panels, the last of one column
    assert (m * m + BLOCK - 1) // BLOCK > 1 and all(np.all(c == 2) for c in per_col["panel"])
    _, K, n, m, q, _ = shape["group-of-3"]
    assert K == 3 and [int(r[0]) for r in per_row["group-of-3"]] == [1, 2, m]
    assert all(np.all(r == r[0]) for r in per_row["group-of-3"]) and len({int(A.astype(bool).sum()) for A in mats["group-of-3"]}) == 3
    forms = [shape[k][4] for k in ("full-none", "full-dense", "full-parts")]
    assert forms[0] is None and forms[1] == "dense" and isinstance(forms[2], tuple)
    for k in ("full-none", "full-dense", "full-parts"):
        assert shape[k][1:4] == (1, 33, 6) and np.all(mats[k][0] != 0)
    # the panel rule at its ends
    assert panel_cols(1, 1) == PANEL_MAX and panel_cols(2 ** 20, 1) == 16 and panel_cols(2 ** 24, 4) == PANEL_MIN
    # signs: what the bounds lean on
    for r in ROWS:
        for cn in make_problem(r, "well")[0]:
            p = cn["parts"]
            if p is not None:
                assert p["S"] is None or np.all(p["S"][2] >= 0)
                assert p["F"] is None or (np.all(p["F"] >= 0) and np.all(p["sigma"] >= 0))
