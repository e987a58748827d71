"""Quadratic cones whose Q = S + F diag(sigma) F' is given by its parts (cxk_add_quadratic_structured): the rows of
test_gpu_quad_structured.py / test_quad_structured_reference.py, their data, the reference restated on operators, and
the context class that lets test_gpu_cone_kernel_matrix.run_rows / build serve unchanged.  numpy only.

Data.  A cone is the dict km.make_cone makes for kind "quad", plus cn["parts"] = dict(S=(indptr, indices, data) or
None, F=(n, r) or None, sigma=(r,) or None).  cn["Q"] is the expansion S + F diag(sigma) F' computed in np.longdouble
(an ExpandedQ: the array carries its parts); cone_reference converts its inputs with ld(), so the expansion's own
rounding is not charged to the kernels.

Signs.  In every row checked against the bounds the entries of S, F and sigma are nonnegative, and S is diagonally
dominant with a positive diagonal (Q > 0).  Then |Q| = |S| + |F| |sigma| |F|', and the magnitudes the reference derives
from |Q| are those of the structured evaluation too.  With mixed signs the reference's magnitudes would be too small and
the test would blame correct code.

Every row is the smallest shape at which its edge exists; test_rows_sit_on_their_edges recomputes each edge with the
launch site's arithmetic.
"""
import numpy as np

import cone_reference as ref
from conex_amd import KktContext
from conex_amd import synthetic as syn

LD = ref.LD

ROW_TILE = 256       # kQuadStreamRowTile: rows per workgroup of quad_struct_rows
T_CHUNK = 64         # kQuadStructTChunk: entries of t staged in LDS at a time
MIN_SEGMENT = 1024   # kQuadFactorMinSegment (cone_route.h)
BLOCK = 256          # kQuadStreamBlock
ONE_LANE_MAX_MEAN = 27      # kQuadCsrOneLaneMaxMean
EIGHT_LANES_MAX_MEAN = 243  # kQuadCsrEightLanesMaxMean

# (id, K, n, m, S, rank)
ROWS = [
    ("min-s", 1, 1, 1, "diagonal", 0),            # smallest, sparse only
    ("min-f", 1, 1, 1, None, 1),                  # smallest, factors only
    ("chol", 1, 40, 3, None, 40),                 # no S; Q = F F', F square nonnegative with a dominant diagonal
    ("row-tile", 1, 257, 3, "tridiagonal", 3),    # one row past a 256-row tile; y eight times the usual (short step)
    ("t-chunk", 1, 130, 2, "diagonal", 65),       # one factor past the 64-entry LDS chunk of t
    ("empty-rows", 1, 20, 4, "even-diagonal", 20),  # rows of S without a nonzero; F carries definiteness
    ("arrow", 1, 300, 3, "arrow", 2),             # one row of 300 nonzeros beside rows of 2 (run under each lane count)
    ("group-of-3", 3, 300, 5, "bands", 4),        # bands of width 1, 2, 4: members of one group with different nnz
    ("m65", 2, 64, 65, "tridiagonal", 1),         # seventeen blocks of the Schur block; T = S A1 with many columns
    ("segments", 1, 4096, 2, "tridiagonal", 2),   # the factor dots split into row segments
    ("duplicates", 1, 33, 2, "duplicates", 1),    # every entry stored twice at half its value
]
ROW_IDS = [r[0] for r in ROWS]
SHORT_STEP_ROWS = ("row-tile",)
LANES = (1, 8, 64)


# ------------------------------------------------------------------------------------ launch arithmetic, restated
def csr_lanes(nnz, rows):
    """QuadCsrLanes (cone_route.h), restated."""
    mean = nnz / rows if rows > 0 else 0.0
    return 1 if mean <= ONE_LANE_MAX_MEAN else 8 if mean <= EIGHT_LANES_MAX_MEAN else 64


def factor_segments(n, columns):
    """QuadFactorSegments (cone_route.h), restated: columns = cones x rank."""
    cols = max(columns, 1)
    return max(1, min(n // MIN_SEGMENT, (512 + cols - 1) // cols))


# ------------------------------------------------------------------------------------ the parts
def csr_from_dense(M):
    """(indptr, indices, data) of the nonzeros of a dense matrix, columns ascending."""
    M = np.asarray(M, dtype=np.float64)
    mask = M != 0
    indptr = np.r_[0, np.cumsum(mask.sum(axis=1))].astype(np.int32)
    rows, cols = np.nonzero(mask)
    return indptr, cols.astype(np.int32), M[rows, cols].copy()


def banded(rng, n, width):
    """(indptr, indices, data) of a symmetric nonnegative band matrix, `width` sub-diagonals, strictly diagonally
    dominant with a diagonal in [2, 3]: built by diagonals, so that n = 50 000 costs nothing."""
    offs = [rng.uniform(0.0, 1.0, n - k) / (2.0 * width) for k in range(1, width + 1) if n - k > 0]
    diag = rng.uniform(2.0, 3.0, n)
    idx, val = [], []
    for i_off, o in enumerate(offs, start=1):
        r = np.arange(n - i_off)
        idx += [np.stack([r + i_off, r]), np.stack([r, r + i_off])]
        val += [o, o]
    idx.append(np.stack([np.arange(n), np.arange(n)]))
    val.append(diag)
    rc = np.concatenate(idx, axis=1)
    v = np.concatenate(val)
    order = np.lexsort((rc[1], rc[0]))
    rows, cols, v = rc[0][order], rc[1][order], v[order]
    indptr = np.r_[0, np.cumsum(np.bincount(rows, minlength=n))].astype(np.int32)
    return indptr, cols.astype(np.int32), v


def make_s(kind, n, member, rng):
    if kind is None:
        return None
    if kind == "diagonal":
        return csr_from_dense(np.diag(rng.uniform(1.0, 2.0, n)))
    if kind == "tridiagonal":
        return banded(rng, n, 1)
    if kind == "bands":
        return banded(rng, n, (1, 2, 4)[member])
    if kind == "even-diagonal":
        d = rng.uniform(1.0, 2.0, n)
        d[1::2] = 0.0
        return csr_from_dense(np.diag(d))
    if kind == "arrow":
        M = np.diag(rng.uniform(1.0, 2.0, n))
        edge = rng.uniform(0.1, 1.0, n - 1) / n
        M[0, 1:], M[1:, 0], M[0, 0] = edge, edge, 2.0
        return csr_from_dense(M)
    if kind == "duplicates":
        indptr, indices, data = banded(rng, n, 1)
        return (2 * indptr).astype(np.int32), np.repeat(indices, 2), np.repeat(0.5 * data, 2)
    raise ValueError(kind)


def make_f(n, rank, rng):
    """Nonnegative factors; a square F gets a dominant diagonal, so that F F' is positive definite on its own."""
    if rank == 0:
        return None
    F = rng.uniform(0.0, 1.0, (n, rank)) / np.sqrt(n)
    if rank == n:
        F = F / np.sqrt(n) + np.diag(rng.uniform(1.0, 2.0, n))
    return F


def nnz_of(parts):
    return 0 if parts["S"] is None else int(parts["S"][0][-1])


# ------------------------------------------------------------------------------------ operators, in longdouble
def _csr_apply(S, X, absolute):
    indptr, indices, data = S
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    d = ref.ld(data)
    if absolute:
        d = np.abs(d)
    out = np.zeros((n,) + X.shape[1:], dtype=LD)
    np.add.at(out, rows, (d[:, None] * X[indices]) if X.ndim == 2 else d * X[indices])
    return out


def _apply(parts, X, absolute):
    X = ref.ld(X)
    out = np.zeros(X.shape, dtype=LD)
    if parts["S"] is not None:
        out = out + _csr_apply(parts["S"], X, absolute)
    if parts["F"] is not None:
        F = ref.ld(parts["F"])
        sg = np.ones(F.shape[1], dtype=LD) if parts["sigma"] is None else ref.ld(parts["sigma"])
        if absolute:
            F, sg = np.abs(F), np.abs(sg)
        t = F.T @ X
        out = out + F @ (sg[:, None] * t if X.ndim == 2 else sg * t)
    return out


def apply_q(parts, X):
    """Q X = S X + F (sigma o (F' X)) in longdouble, Q never formed."""
    return _apply(parts, X, False)


def apply_abs_q(parts, X):
    """(|S| + |F| |sigma| |F|') X: what |Q| X is when the parts do not cancel."""
    return _apply(parts, X, True)


class ExpandedQ(np.ndarray):
    """The expansion of a structured Q, carrying the parts it came from."""
    parts = None

    def __array_finalize__(self, obj):
        self.parts = getattr(obj, "parts", None)


def expand(parts, n):
    """S + F diag(sigma) F' as an n x n longdouble matrix (small n only)."""
    Q = np.zeros((n, n), dtype=LD)
    if parts["S"] is not None:
        indptr, indices, data = parts["S"]
        rows = np.repeat(np.arange(n), np.diff(indptr))
        np.add.at(Q, (rows, indices), ref.ld(data))
    if parts["F"] is not None:
        F = ref.ld(parts["F"])
        sg = np.ones(F.shape[1], dtype=LD) if parts["sigma"] is None else ref.ld(parts["sigma"])
        Q += (F * sg) @ F.T
    out = Q.view(ExpandedQ)
    out.parts = parts
    return out


def quad_schur_op(A, c, W, parts):
    """cone_reference.quad_schur restated on the operators apply_q / apply_abs_q, for orders at which Q cannot be
    expanded: G, AW, AQc and the two scalars, each with its magnitude (g = 1)."""
    A, c, W = ref.ld(A), ref.ld(c), ref.ld(W)
    aA, ac, aW = np.abs(A), np.abs(c), np.abs(W)
    A0, A1, a0, a1 = A[0], A[1:], aA[0], aA[1:]
    qw, qwm = apply_q(parts, W[1:]), apply_abs_q(parts, aW[1:])
    qc, qcm = apply_q(parts, c[1:]), apply_abs_q(parts, ac[1:])
    det, detm = W[0] * W[0] - W[1:] @ qw, W[0] * W[0] + aW[1:] @ qwm
    scale, scalem = qw @ c[1:] + c[0] * W[0], qwm @ ac[1:] + ac[0] * aW[0]
    v, vm = A1.T @ qw + A0 * W[0], a1.T @ qwm + a0 * aW[0]
    gram, gramm = A1.T @ apply_q(parts, A1), a1.T @ apply_abs_q(parts, a1)
    t, tm = np.outer(A0, A0) - gram, np.outer(a0, a0) + gramm
    G = 2 * (-det * t + 2 * np.outer(v, v))
    Gm = 2 * (ref.mulm(det, detm, t, tm) + 2 * ref.mulm(v[:, None], vm[:, None], v[None, :], vm[None, :]))
    r, rm = A1.T @ qc - A0 * c[0], a1.T @ qcm + a0 * ac[0]
    AQc = 2 * (det * r + 2 * v * scale)
    AQcm = 2 * (ref.mulm(det, detm, r, rm) + 2 * ref.mulm(v, vm, scale, scalem))
    z, zm = c[1:] @ qc - c[0] * c[0], ac[1:] @ qcm + c[0] * c[0]
    s1 = 2 * (det * z + 2 * scale * scale)
    s1m = 2 * (ref.mulm(det, detm, z, zm) + 2 * ref.mulm(scale, scalem, scale, scalem))
    return dict(G=(G, Gm), AW=(2 * v, 2 * vm), AQc=(AQc, AQcm), sc=(ref.ld([2 * scale, s1]), ref.ld([2 * scalem, s1m])), g=1.0)


# ------------------------------------------------------------------------------------ problems
def make_parts(s_kind, n, rank, member, rng):
    return dict(S=make_s(s_kind, n, member, rng), F=make_f(n, rank, rng), sigma=None if rank == 0 else rng.uniform(0.5, 1.5, rank))


def make_cone(n, m, parts, point, rng):
    """km.make_cone's quadratic cone around the given parts."""
    c = 0.2 * rng.uniform(-1, 1, n + 1)
    c[0] = 1.0
    Q = expand(parts, n)
    return dict(kind="quad", m=m, A=rng.uniform(-1, 1, (n + 1, m)), c=c, Q=Q, parts=parts,
                W=ref.spin_scaling_point(rng, n, point, np.asarray(Q, dtype=np.float64)))


def row_seed(row):
    _, K, n, m, _, rank = row
    return 9000 + 31 * n + 7 * m + K + 3 * rank


def make_problem(row, point, seed=None):
    """(cones, cliques, num_vars): K structured cones in a chain of cliques, as km.make_problem arranges them."""
    _, K, n, m, s_kind, rank = row
    rng = np.random.default_rng(row_seed(row) if seed is None else seed)
    cliques, num_vars = syn.chain_cliques(K, m, 1 if m > 1 else 0)
    return [make_cone(n, m, make_parts(s_kind, n, rank, k, rng), point, rng) for k in range(K)], cliques, num_vars


def row_parts(row):
    """The parts of a row's cones alone (what the edges depend on), without expanding Q."""
    _, K, n, m, s_kind, rank = row
    rng = np.random.default_rng(row_seed(row))
    return [make_parts(s_kind, n, rank, k, rng) for k in range(K)]


class StructuredQuad(KktContext):
    """A KktContext whose add_quadratic hands the parts behind an ExpandedQ to add_quadratic_structured; any other Q
    goes where it always went."""

    def add_quadratic(self, Q, A, c, vars_=None):
        parts = getattr(Q, "parts", None)
        if parts is None:
            return super().add_quadratic(Q, A, c, vars_)
        return self.add_quadratic_structured(parts["S"], parts["F"], parts["sigma"], A, c, vars_)


# ------------------------------------------------------------------------------------ the edges
def test_rows_sit_on_their_edges():
    shape = {r[0]: r for r in ROWS}
    parts = {r[0]: row_parts(r) for r in ROWS}
    _, K, n, m, s, rank = shape["min-s"]
    assert (n, m, rank) == (1, 1, 0) and nnz_of(parts["min-s"][0]) == 1
    _, K, n, m, s, rank = shape["min-f"]
    assert (n, m, rank) == (1, 1, 1) and s is None
    _, K, n, m, s, rank = shape["chol"]
    assert s is None and rank == n
    _, K, n, m, s, rank = shape["row-tile"]
    assert n % ROW_TILE == 1 and n > ROW_TILE and "row-tile" in SHORT_STEP_ROWS
    _, K, n, m, s, rank = shape["t-chunk"]
    assert rank == T_CHUNK + 1
    _, K, n, m, s, rank = shape["empty-rows"]
    ptr = parts["empty-rows"][0]["S"][0]
    assert np.all(np.diff(ptr)[1::2] == 0) and np.all(np.diff(ptr)[0::2] == 1) and rank == n
    _, K, n, m, s, rank = shape["arrow"]
    ptr = parts["arrow"][0]["S"][0]
    per_row = np.diff(ptr)
    assert per_row[0] == n and np.all(per_row[1:] == 2) and n > 4 * 64  # the long row wraps 64 lanes more than four times
    assert csr_lanes(ptr[-1], n) == 1  # the rule sees the mean: the long row rides one lane unless the width is forced
    _, K, n, m, s, rank = shape["group-of-3"]
    counts = [nnz_of(p) for p in parts["group-of-3"]]
    assert K == 3 and len(set(counts)) == 3 and n > ROW_TILE
    assert csr_lanes(sum(counts), K * n) == 1
    _, K, n, m, s, rank = shape["m65"]
    assert (m * m + BLOCK - 1) // BLOCK == 17 and m * m % BLOCK != 0 and m % 4 == 1  # (four columns of T per thread)
    _, K, n, m, s, rank = shape["segments"]
    assert factor_segments(n, K * rank) == 4 and factor_segments(2 * MIN_SEGMENT - 1, K * rank) == 1
    assert all(factor_segments(r[2], r[1] * r[5]) == 1 for r in ROWS if r[0] != "segments")
    _, K, n, m, s, rank = shape["duplicates"]
    ptr, idx, val = parts["duplicates"][0]["S"]
    assert np.all(idx[0::2] == idx[1::2]) and np.all(val[0::2] == val[1::2]) and np.all(np.diff(ptr) % 2 == 0)
    # the lanes rule at its cut points
    assert [csr_lanes(k * 100, 100) for k in (0, 27, 28, 243, 244)] == [1, 1, 8, 8, 64]
    # signs: what the bounds lean on
    for plist in parts.values():
        for p in plist:
            assert p["S"] is None or np.all(p["S"][2] >= 0)
            assert p["F"] is None or (np.all(p["F"] >= 0) and np.all(p["sigma"] >= 0))
