"""Rows, references and the float64 model shared by test_lmi_hermitian_factored_reference.py (CPU) and
test_gpu_lmi_hermitian_factored.py: Hermitian matrix inequalities over R / C / H given by factors
(KktContext.add_hermitian_factored, kernels_lmi_factored.hip.h).

A row is a problem of synthetic.factored_hermitian_problem.  The comparison is the LMI matrix's: |x - ref| <= c u M
entry by entry, ref = lmi_reference.py with its d argument in longdouble on the EXPANDED planes A_i, the constants those
of test_gpu_lmi_kernel_matrix.py.  M is the magnitude of the expression the kernels evaluate, e.g.
sum |sigma_k sigma_l| sum_p (|L_p|' |W| |F0|)_kl^2 for G.  The planes of one term f f^* already cancel (plane 0 is
sum_p f_p f_p'), so |A_i| understates it at every rank: every row takes its magnitudes from
A~_i = sum_k |sigma_k| |f_k| |f_k|^* with every plane product taken in absolute values (absolute_expansion), whose
lmi_reference magnitudes are sums over the same absolute products as the factored expressions.  This is
lmi_factored_cases.magnitude_matrices for its `cancelling` rows.
"""
import numpy as np

import lmi_reference as ref
from conex_amd import synthetic as syn
from test_gpu_lmi_kernel_matrix import C_WEIGHT, scaling_points, slack_norm

LD = ref.LD


def _row3(d, seed):
    """Three members of one group (n = 7, m = 6, R = 9) with their own rank_ptr and sigma."""
    rng = np.random.default_rng(seed)
    out = []
    for ranks in ([2, 1, 1, 3, 1, 1], [1, 0, 4, 1, 2, 1], [1, 1, 1, 1, 0, 5]):
        out.append((rng.standard_normal((d, 7, 9)), np.concatenate([[0], np.cumsum(ranks)]), rng.choice([-1.0, 1.0], 9)))
    return out


def _both(name, **kw):
    return {f"{name}-d{d}": dict(d=d, **kw) for d in (2, 4)}


# name -> problem keywords
ROWS = {
    **_both("n1-ranks-1-2", K=1, n=1, ranks=(1, 2)),                               # N = d
    **_both("n5-ranks-3-1-0-2", K=1, n=5, ranks=(3, 1, 0, 2), signs="mixed"),      # an empty variable, block sums
    "n17-d4": dict(K=1, n=17, d=4, ranks=(1, 2, 1)),                               # N = 68: past the 64-lane stride
    "n33-d2": dict(K=1, n=33, d=2, ranks=(1, 2, 1)),                               # N = 66
    **_both("n6-m17-rank1", K=2, n=6, ranks=(1,) * 17, signs="mixed"),             # m^2 > 256: G spans two workgroups
    **_both("n8-R65", K=1, n=8, ranks=(13,) * 5, signs="matrix"),                  # more than one GEMM tile of P per plane
    "n7-three-members-d2": dict(K=3, n=7, d=2, factors=_row3(2, 5)),
    "n7-three-members-d4": dict(K=3, n=7, d=4, factors=_row3(4, 6)),
    "n9-d1": dict(K=1, n=9, d=1, ranks=(2, 1, 0, 3), signs="mixed"),
}


def make_row(name, seed=11):
    return syn.factored_hermitian_problem(branching=2, overlap=2, seed=seed, **ROWS[name])


def row_seed(name):
    return 31 + list(ROWS).index(name)


def conj_transpose(X):
    T = np.swapaxes(X, -1, -2).copy()
    T[1:] = -T[1:]
    return T


def absolute_expansion(prob, c):
    """A~_i = sum_k |sigma_k| |f_k| |f_k|^* of member c, every plane product in absolute values: (m, d, n, n)."""
    F, ptr, sg = np.abs(prob["F"][c]), prob["rank_ptr"][c], np.abs(prob["sigma"][c])
    d, n, m = F.shape[0], F.shape[1], len(ptr) - 1
    A = np.zeros((m, d, n, n))
    for i in range(m):
        for k in range(ptr[i], ptr[i + 1]):
            f = F[:, :, k:k + 1]
            A[i] += sg[k] * np.asarray(ref.hc_mul_abs(f, np.swapaxes(f, -1, -2)), dtype=np.float64)
    return A


def direction(prob, seed):
    """y with C - sum y_i A_i positive definite for every member (||sum y_i A_i|| <= 0.5; C is I + a small term)."""
    rng = np.random.default_rng(seed + 1)
    y = rng.uniform(-1, 1, prob["num_vars"])
    nrm = max(slack_norm(prob["A"][c], y[cl], prob["d"]) for c, cl in enumerate(prob["cliques"]))
    return y * (0.5 / max(nrm, 1e-300))


def points(prob, point, seed):
    return scaling_points(point, len(prob["cliques"]), prob["n"], prob["d"], seed)


# The (row, point) pairs at which the device's converged Ritz value may miss run_point's TOL_LANCZOS against the
# oracle because the run is not determined by its input: none.
LMAX_EXEMPT = set()


# ---- references: values from the expanded planes, magnitudes of the factored expressions
def ref_schur(prob, c, W):
    d = prob["d"]
    r = ref.schur(prob["A"][c], prob["C"][c], W, d)
    rm = ref.schur(absolute_expansion(prob, c), prob["C"][c], W, d)
    return {key: (r[key][0], rm[key][1]) for key in r}


def ref_prepare(prob, c, W, z):
    d = prob["d"]
    r = ref.prepare(prob["A"][c], prob["C"][c], W, z, C_WEIGHT, d)
    rm = ref.prepare(absolute_expansion(prob, c), prob["C"][c], W, z, C_WEIGHT, d)
    return {key: (r[key][0], rm[key][1]) for key in r}


def ref_affine(prob, c, W, z, e_weight):
    d = prob["d"]
    Wa = ref.affine(prob["A"][c], prob["C"][c], W, z, C_WEIGHT, e_weight, d)[0]
    Wm = ref.affine(absolute_expansion(prob, c), prob["C"][c], W, z, C_WEIGHT, e_weight, d)[1]
    return Wa, Wm


def ref_take_step(prob, c, W, z, e_weight, step):
    """lmi_reference.take_step (Taylor form, growth 1); its magnitude sym(|F|^4 |W|) reads only the magnitude of WS,
    which comes from A~."""
    d = prob["d"]
    Wn, _, growth = ref.take_step(prob["A"][c], prob["C"][c], W, z, C_WEIGHT, e_weight, step, d)
    Wm = ref.take_step(absolute_expansion(prob, c), prob["C"][c], W, z, C_WEIGHT, e_weight, step, d)[1]
    return Wn, Wm, growth


# ---- the folded expressions in float64, in the kernels' summation orders
def embed(X):
    """The real representation L(X) of d planes of r x c: block (k, j) = HC_SIGN[k ^ j, j] X_{k ^ j}; (d r) x (d c)."""
    X = np.asarray(X, dtype=np.float64)
    d = X.shape[0]
    return np.block([[syn.HC_SIGN[k ^ j, j] * X[k ^ j] for j in range(d)] for k in range(d)])


def extract(L, d):
    """The planes of a real representation: block (k, 0) is plane k."""
    n = L.shape[0] // d
    return np.stack([L[k * n:(k + 1) * n, :L.shape[1] // d] for k in range(d)])


def model_products(F, W):
    """(L(F), Z = L(W) F0, P = L(F)' Z as d planes of R x R)."""
    d, _, R = F.shape
    LF = embed(F)
    Z = embed(W) @ LF[:, :R]
    return LF, Z, (LF.T @ Z).reshape(d, R, R)


def model_schur(F, ptr, sigma, C, W):
    """G (lower triangle), AW, AQc, the two scalars as kernels_lmi_factored.hip.h forms them for d planes: Z = W F0,
    P = L(F)' Z, Y = C Z and X = W (C W) as float64 products (the GEMM's own order inside a dot product is not
    restated), the plane squares added plane 0 first, the block sums l inside k ascending, only P_p(k, l) with k >= l
    read, every contraction tr / d.  numpy has no fma: products are rounded."""
    d, _, R = F.shape
    m = len(ptr) - 1
    LF, Z, P = model_products(F, W)
    LC, LW = embed(C), embed(W)
    Y = LC @ Z
    sq = np.zeros((R, R))
    for p in range(d):
        sq = P[p] * P[p] + sq
    G = np.zeros((m, m))
    for i in range(m):
        for j in range(i + 1):
            acc = 0.0
            for k in range(ptr[i], ptr[i + 1]):
                row = 0.0
                for l in range(ptr[j], ptr[j + 1]):
                    row = sigma[l] * (sq[k, l] if k >= l else sq[l, k]) + row
                acc = sigma[k] * row + acc
            G[i, j] = acc
    AW, AQ = np.zeros(m), np.zeros(m)
    for i in range(m):
        for k in range(ptr[i], ptr[i + 1]):
            AQ[i] = sigma[k] * float(Z[:, k] @ Y[:, k]) + AQ[i]
            AW[i] = sigma[k] * P[0, k, k] + AW[i]
    X = LW @ (LC @ LW)
    return G, AW, AQ, np.array([np.sum(LC * LW), np.sum(LC * X)]) / d


def model_slack(F, ptr, sigma, C, z, c_weight):
    """S = L(F) diag(sigma_k y_i(k), once per column block) L(F)' - k L(C), of order d n."""
    d = F.shape[0]
    var = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    LF = embed(F)
    return -(c_weight * embed(C)) + (LF * np.tile(sigma * z[var], d)) @ LF.T


def model_step(S, W, e_weight, step):
    """(normsqrd, frob, trace, W after TakeStep, WS) of the large-order route's Hermitian branch on S (order d n): traces
    are tr / d, the rank is the hyper-complex order, E = ((I + X/4 + X (X/4)/8)^2)^2."""
    d = W.shape[0]
    LW = embed(W)
    N = len(LW)
    WS = LW @ S
    frob, t = float(np.sum(WS * WS.T)) / d, float(np.trace(WS)) / d
    X = (WS + e_weight * np.eye(N)) * step
    Xq = X / 4
    Y = np.eye(N) + Xq + (X @ Xq) / 8
    Y = Y @ Y
    EW = (Y @ Y) @ LW
    return frob + 2 * t + N // d, frob, -t, extract(0.5 * (EW + EW.T), d), WS


def model_affine(WS, W, e_weight):
    LW = embed(W)
    return extract(LW * (1 + e_weight) + WS @ LW, W.shape[0])


def ratio(x, val, mag, c):
    """max |x - val| / (c u M): at most 1 where the bound holds."""
    err = np.abs(np.asarray(x, dtype=np.float64).astype(LD) - val)
    bound = c * ref.U64 * np.asarray(mag, dtype=LD)
    return float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
