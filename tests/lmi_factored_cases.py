"""Rows, references and the float64 model shared by test_lmi_factored_reference.py (CPU) and
test_gpu_lmi_factored.py: LMIs given by factors (KktContext.add_lmi_factored, kernels_lmi_factored.hip.h).

A row is a problem of synthetic.factored_lmi_problem.  The comparison is the LMI matrix's: |x - ref| <= c u M entry
by entry, ref = lmi_reference.py in longdouble on the EXPANDED A_i, the constants those of
test_gpu_lmi_kernel_matrix.py.  M is the magnitude of the expression the kernels evaluate, e.g.
sum |sigma_k sigma_l| (|f_k|' |W| |f_l|)^2 for G.  Where the terms of an A_i do not cancel (one sign of sigma and
non-negative or disjoint-support vectors within it, or rank one) that is lmi_reference's own magnitude of the
expanded data; rows marked `cancelling` take it from  A~_i = sum_k |sigma_k| |f_k| |f_k|'  instead, whose
lmi_reference magnitudes are exactly the factored ones (magnitude_matrices).
"""
import numpy as np

import lmi_reference as ref
from conex_amd import synthetic as syn
from test_gpu_lmi_kernel_matrix import C_WEIGHT, scaling_points

LD = ref.LD


def theta_pairs(n, m, seed):
    """The Lovasz theta pairs 1/2 [(e_i + e_j)(e_i + e_j)' - (e_i - e_j)(e_i - e_j)'] = e_i e_j' + e_j e_i' in a
    random orthonormal basis: rank 2, sigma = (+1/2, -1/2), dense vectors whose terms cancel."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    F = np.zeros((n, 2 * m))
    for t in range(m):
        i, j = sorted(rng.choice(n, 2, replace=False))
        F[:, 2 * t] = Q[:, i] + Q[:, j]
        F[:, 2 * t + 1] = Q[:, i] - Q[:, j]
    return F, np.arange(0, 2 * m + 1, 2), np.tile([0.5, -0.5], m)


def identity_first(n, m, seed):
    """Variable 0 is the identity (rank n, columns e_k: the t I of a design program), the others rank one."""
    rng = np.random.default_rng(seed)
    F = np.hstack([np.eye(n), rng.standard_normal((n, m - 1))])
    return F, np.concatenate([[0], np.arange(n, n + m)]), None


def _row3(seed):
    """Three members of one group (n = m = R = 13): rank one; ranks (2, 0, 1, ..); ranks (.., 1, 0, 2); own signs."""
    rng = np.random.default_rng(seed)
    out = []
    for ranks in ([1] * 13, [2, 0] + [1] * 11, [1] * 11 + [0, 2]):
        F = rng.uniform(0.0, 1.0, (13, 13))
        sg = np.repeat(rng.choice([-1.0, 1.0], 13), ranks)
        out.append((F, np.concatenate([[0], np.cumsum(ranks)]), sg))
    return out


# name -> (problem keywords, cancelling)
ROWS = {
    "n2-m1-rank1": (dict(K=1, n=2, ranks=(1,)), False),
    "n5-ranks-1-2-0": (dict(K=1, n=5, ranks=(1, 2, 0), nonneg=True), False),
    "n13-three-members": (dict(K=3, n=13, factors=_row3(5)), False),
    "n20-ranks-3-1-4-1-5-9": (dict(K=1, n=20, ranks=(3, 1, 4, 1, 5, 9), nonneg=True, signs="matrix"), False),
    "n12-theta-pairs": (dict(K=1, n=12, factors=[theta_pairs(12, 8, 6)]), True),
    "n16-identity-first": (dict(K=1, n=16, factors=[identity_first(16, 5, 7)]), False),
    "n64-m65-rank1": (dict(K=2, n=64, ranks=(1,) * 65, signs="mixed"), False),
    "n70-m40-R129": (dict(K=1, n=70, ranks=(4,) * 29 + (1,) * 10 + (3,), nonneg=True, signs="matrix"), False),
    "n66-m257-rank1": (dict(K=1, n=66, ranks=(1,) * 257), False),
}


def make_row(name, seed=11):
    kw, cancelling = ROWS[name]
    prob = syn.factored_lmi_problem(branching=2, overlap=2, seed=seed, **kw)
    prob["cancelling"] = cancelling
    return prob


def absolute_expansion(prob, c):
    """A~_i = sum_k |sigma_k| |f_k| |f_k|' of member c."""
    return syn.expand_factors(np.abs(prob["F"][c]), prob["rank_ptr"][c], np.abs(prob["sigma"][c]))


def magnitude_matrices(prob, c):
    return absolute_expansion(prob, c) if prob["cancelling"] else prob["A"][c]


def direction(prob, seed):
    """y with C - sum y_i A_i positive definite for every member (||sum y_i A_i|| <= 0.5; C is I + a small term)."""
    rng = np.random.default_rng(seed + 1)
    y = rng.uniform(-1, 1, prob["num_vars"])
    nrm = max(np.linalg.norm(np.tensordot(y[cl], prob["A"][c], axes=1), 2) for c, cl in enumerate(prob["cliques"]))
    return y * (0.5 / max(nrm, 1e-300))


def points(prob, point, seed):
    return scaling_points(point, len(prob["cliques"]), prob["n"], 0, seed)


# The one (row, point) at which the device's converged Ritz value misses run_point's TOL_LANCZOS against the oracle
# (8.5e-6 of the spectral radius, measured on the MI355X; every other row and point holds it): the query's Lanczos run
# is not determined by its input there (dominant_end_spread), and test_gpu_lmi_factored.py runs the expanded data
# through add_lmi at that point beside it.
LMAX_EXEMPT = {("n64-m65-rank1", 1e6)}


def dominant_end_spread(prob, W, z, spec, trials=12):
    """Largest change, over the members, of the query's converged Ritz value (the end of largest magnitude) when the
    entries of WS change by one unit roundoff: the float64 recurrence of lmi_reference.two_sided_lanczos, measured as
    lmi_reference.ritz_spread measures both ends."""
    rng = np.random.default_rng(0)
    spread = 0.0
    for c in range(len(W)):
        WS, _, S = ref.weighted_slack(prob["A"][c], prob["C"][c], W[c], z[c], C_WEIGHT, 0)
        WS, S = np.asarray(WS[0], dtype=np.float64), np.asarray(S[0], dtype=np.float64)
        n = len(WS)
        r = S[:, int(np.argmax(np.diag(WS)))]
        end = int(abs(spec[c][1]) > abs(spec[c][0]))
        base = ref.two_sided_lanczos(WS, W[c], r, n // 2)[end]
        for _ in range(trials):
            P = WS * (1 + ref.U64 * rng.choice([-1.0, 1.0], WS.shape))
            spread = max(spread, abs(ref.two_sided_lanczos(P, W[c], r, n // 2)[end] - base))
    return spread


# ---- references: values from the expanded A, magnitudes of the factored expressions
def ref_schur(prob, c, W):
    r = ref.schur(prob["A"][c], prob["C"][c], W, 0)
    if prob["cancelling"]:
        rm = ref.schur(magnitude_matrices(prob, c), prob["C"][c], W, 0)
        r = {key: (r[key][0], rm[key][1]) for key in r}
    return r


def ref_prepare(prob, c, W, z):
    r = ref.prepare(prob["A"][c], prob["C"][c], W, z, C_WEIGHT, 0)
    if prob["cancelling"]:
        rm = ref.prepare(magnitude_matrices(prob, c), prob["C"][c], W, z, C_WEIGHT, 0)
        r = {key: (r[key][0], rm[key][1]) for key in r}
    return r


def ref_affine(prob, c, W, z, e_weight):
    Wa, Wm = ref.affine(prob["A"][c], prob["C"][c], W, z, C_WEIGHT, e_weight, 0)
    if prob["cancelling"]:
        Wm = ref.affine(magnitude_matrices(prob, c), prob["C"][c], W, z, C_WEIGHT, e_weight, 0)[1]
    return Wa, Wm


def ref_take_step(prob, c, W, z, e_weight, step):
    """lmi_reference.take_step; a cancelling row restates its magnitude sym((|E| + |E| |X|) |W|) with |X| from A~."""
    Wn, Wm, growth = ref.take_step(prob["A"][c], prob["C"][c], W, z, C_WEIGHT, e_weight, step, 0)
    if prob["cancelling"]:
        n = prob["n"]
        WS = ref.weighted_slack(prob["A"][c], prob["C"][c], W, z, C_WEIGHT, 0)[0]
        mWS = ref.weighted_slack(magnitude_matrices(prob, c), prob["C"][c], W, z, C_WEIGHT, 0)[1]
        I = ref.eye_planes(0, n)
        X = (WS + LD(e_weight) * I) * LD(step)
        mX = (mWS + abs(LD(e_weight)) * I) * abs(LD(step))
        X2 = X[0] @ X[0]
        Um = X[0] @ (X2 + 60 * np.eye(n, dtype=LD))
        V = 12 * X2 + 120 * np.eye(n, dtype=LD)
        E = ref.lu_solve(V - Um, V + Um)[None]
        Tm = ref.hc_mul_abs(np.abs(E) + ref.hc_mul_abs(E, mX), ref.planes(W, 0))
        Wm = ((Tm + np.swapaxes(Tm, -1, -2)) / 2)[0]
    return Wn, Wm, growth


# ---- the factored expressions in float64, in the kernels' summation orders
def model_schur(F, ptr, sigma, C, W):
    """G (lower triangle), AW, AQc, the two scalars as kernels_lmi_factored.hip.h forms them: Z = W F, P = F' Z,
    Y = C Z and X = W (C W) as float64 products (the GEMM's own order inside a dot product is not restated), the
    block sums l inside k ascending, only P(k, l) with k >= l read.  numpy has no fma: products are rounded."""
    R, m = F.shape[1], len(ptr) - 1
    Z = W @ F
    P = np.tril(F.T @ Z)
    Y = C @ Z
    G = np.zeros((m, m))
    if all(ptr[i + 1] - ptr[i] == 1 for i in range(m)):
        G = np.tril((P * P) * np.outer(sigma, sigma))
    else:
        for i in range(m):
            for j in range(i + 1):
                acc = 0.0
                for k in range(ptr[i], ptr[i + 1]):
                    row = 0.0
                    for l in range(ptr[j], ptr[j + 1]):
                        p = P[k, l] if k >= l else P[l, k]
                        row = (sigma[l] * p) * p + row
                    acc = sigma[k] * row + acc
                G[i, j] = acc
    AW, AQ = np.zeros(m), np.zeros(m)
    for i in range(m):
        for k in range(ptr[i], ptr[i + 1]):
            AQ[i] = sigma[k] * float(Z[:, k] @ Y[:, k]) + AQ[i]
            AW[i] = sigma[k] * P[k, k] + AW[i]
    X = W @ (C @ W)
    return G, AW, AQ, np.array([np.sum(C * W), np.sum(C * X)])


def model_slack(F, ptr, sigma, C, z, c_weight):
    """S = Fs F' - k C with Fs = F diag(sigma_k y_i(k))."""
    var = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    return -(c_weight * C) + (F * (sigma * z[var])) @ F.T


def model_step(S, W, e_weight, step):
    """(normsqrd, frob, trace, W after TakeStep, W after the affine update) of the large-order route on S."""
    n = len(W)
    WS = W @ S
    frob, t = float(np.sum(WS * WS.T)), float(np.trace(WS))
    X = (WS + e_weight * np.eye(n)) * step
    X2 = X @ X
    Um = X @ (X2 + 60 * np.eye(n))
    V = 12 * X2 + 120 * np.eye(n)
    EW = np.linalg.solve(V - Um, V + Um) @ W
    return frob + 2 * t + n, frob, -t, 0.5 * (EW + EW.T), WS


def model_affine(WS, W, e_weight):
    return W * (1 + e_weight) + WS @ W


def ratio(x, val, mag, c):
    """max |x - val| / (c u M): at most 1 where the bound holds."""
    err = np.abs(np.asarray(x, dtype=np.float64).astype(LD) - val)
    bound = c * ref.U64 * np.asarray(mag, dtype=LD)
    return float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
