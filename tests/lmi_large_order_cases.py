"""Inputs and float64 restatements shared by test_lmi_large_order_reference.py (CPU) and
test_gpu_lmi_large_order.py (GPU): matrix inequalities beyond the one-workgroup limits of the large-order route
(order 1024 of the Pade LU's panel, order 2549 of the Lanczos run's LDS).

At these orders the longdouble loops of lmi_reference.py take minutes, so the take step is restated in float64
(numpy.linalg.solve for the Pade system); its bound is therefore twice the existing constant.  The Lanczos runs are
kept SHORT by construction: with W = I and a slack "identity plus a few rank-one terms" the Krylov space has as many
dimensions as the slack has distinct eigenvalues, the run breaks there, and its Ritz values are those eigenvalues.
"""
import numpy as np

import lmi_reference as ref
from conex_amd import synthetic as syn
from conex_amd.synthetic import HC_SIGN

U = ref.U64
# the constants tests/test_gpu_lmi_kernel_matrix.py checks these stages with (test_lmi_large_order_reference.py
# asserts that they still are)
C_PREPARE = 64
C_TAKE = 256
TOL_LANCZOS = 1e-6
TOL_SPECTRUM = 1e-12
STABLE = 1e-9
C_WEIGHT = 1.0

RANK_TWO = (0.7, -0.4)                          # eigenvalues of minus_s: -1.7, -0.6 and -1
DOZEN = tuple(np.linspace(-0.4, 0.7, 11))       # eleven more beside -1: twelve distinct eigenvalues

# (id, order, m, shifts, seed): the real short-run inputs of the GPU tests past the LDS ceiling
SHORT_REAL = [("rank-two", 2550, 3, RANK_TWO, 11), ("dozen", 2550, 2, DOZEN, 12)]
# the edge of the launch that sums the partials of a matrix pass (kWideReduceMinOrder = 2049), under mode 1
SHORT_EDGE = [("edge-2048", 2048, 2, RANK_TWO, 14), ("edge-2049", 2049, 2, RANK_TWO, 15)]
SHORT_COMPLEX = ("complex-rank-two", 1275, 3, RANK_TWO, 13)   # real representation of order 2550
# (order, seed) of the long recurrences: the chip-wide run against the one-workgroup run
LONG_REAL = [(64, 3), (65, 4), (127, 3), (130, 4), (200, 3)]   # 200 = 3 x 64 + 8: no multiple of the 64 x 64 tile
LONG_COMPLEX = [(32, 5), (65, 5), (100, 5)]                    # real-representation orders 64, 130, 200


def orthonormal(rng, n, k, complex_=False):
    G = rng.standard_normal((n, k))
    if complex_:
        G = G + 1j * rng.standard_normal((n, k))
    return np.linalg.qr(G)[0]


def short_run_lmi(n, m, shifts, seed):
    """(A, C, y, eigenvalues): sum_i y_i A_i - C = -(I + sum_k shifts[k] u_k u_k') with orthonormal dense u_k.

    Variable 0 carries the positive shifts, variable 1 the negative ones (y = 1 for both after scaling A by the
    shift); further variables hold random symmetric matrices and y = 0."""
    rng = np.random.default_rng(seed)
    sh = np.asarray(shifts, dtype=np.float64)
    Q = orthonormal(rng, n, len(sh))
    A = np.zeros((m, n, n))
    pos, neg = sh > 0, sh < 0
    A[0] = -(Q[:, pos] * sh[pos]) @ Q[:, pos].T
    A[1] = -(Q[:, neg] * sh[neg]) @ Q[:, neg].T
    y = np.zeros(m)
    y[:2] = 1.0
    for i in range(2, m):
        R = syn.random_sym(rng, n)
        A[i] = R / np.linalg.norm(R, 2)
    A = 0.5 * (A + np.swapaxes(A, -1, -2))
    return A, np.eye(n), y, np.sort(np.append(-(1.0 + sh), -1.0))


def short_run_complex(n, m, shifts, seed):
    """The same over C as d = 2 planes: A (m, 2, n, n), C (2, n, n), y, eigenvalues."""
    rng = np.random.default_rng(seed)
    sh = np.asarray(shifts, dtype=np.float64)
    Q = orthonormal(rng, n, len(sh), complex_=True)
    A = np.zeros((m, 2, n, n))
    for slot, mask in ((0, sh > 0), (1, sh < 0)):
        Z = -(Q[:, mask] * sh[mask]) @ Q[:, mask].conj().T
        Z = 0.5 * (Z + Z.conj().T)
        A[slot, 0], A[slot, 1] = Z.real, Z.imag
    y = np.zeros(m)
    y[:2] = 1.0
    for i in range(2, m):
        A[i] = syn.random_hermitian(rng, 2, n)
        A[i] /= np.linalg.norm(ref.complex_rep(A[i], 2), 2)
    Cm = np.zeros((2, n, n))
    Cm[0] = np.eye(n)
    return A, Cm, y, np.sort(np.append(-(1.0 + sh), -1.0))


def minus_s(A, Cm, y, c_weight=C_WEIGHT):
    return np.tensordot(y, A, axes=1) - c_weight * Cm


def lanczos_count(WS, W, r, num_iter):
    """(steps taken before the break, min Ritz, max Ritz) of a float64 run of the reference's real two-sided Lanczos
    (lmi_reference.two_sided_lanczos, which does not report the count)."""
    V0, V1 = W @ r, r.copy()
    nrm = np.sqrt(V0 @ V1)
    V0, V1 = V0 / nrm, V1 / nrm
    U0, U1 = WS @ V0, WS.T @ V1
    alpha, beta = [V0 @ U1], []
    U0, U1 = U0 - alpha[0] * V0, U1 - alpha[0] * V1
    for _ in range(1, num_iter):
        b2 = U0 @ U1
        if not b2 >= 1e-6:
            break
        b = np.sqrt(b2)
        P0, P1, V0, V1 = V0, V1, U0 / b, U1 / b
        U0, U1 = WS @ V0, WS.T @ V1
        a = V0 @ U1
        alpha.append(a)
        beta.append(b)
        U0, U1 = U0 - a * V0 - b * P0, U1 - a * V1 - b * P1
    ev = np.linalg.eigvalsh(np.diag(alpha) + np.diag(beta, 1) + np.diag(beta, -1))
    return len(alpha), float(ev[0]), float(ev[-1])


def start_columns(WS, S):
    """The start vectors of PrepareStep (a column of WS) and of the query (that column of minus_s)."""
    idx = int(np.argmax(np.diag(WS)))
    return WS[:, idx], S[:, idx]


# ------------------------------------------------------------------ the take step in float64
def _planes(X, d):
    X = np.asarray(X, dtype=np.float64)
    return X[None] if d == 0 else X


def hc_mul64(X, Y, absolute=False):
    d = X.shape[0]
    Z = np.zeros((d, X.shape[1], Y.shape[2]))
    for i in range(d):
        for j in range(d):
            if absolute:
                Z[i ^ j] += np.abs(X[i]) @ np.abs(Y[j])
            else:
                Z[i ^ j] += HC_SIGN[i, j] * (X[i] @ Y[j])
    return Z


def weighted_slack64(A, Cm, W, y, c_weight, d):
    Cp, Wp = _planes(Cm, d), _planes(W, d)
    S = -c_weight * Cp
    Sm = abs(c_weight) * np.abs(Cp)
    for i in range(A.shape[0]):
        a = _planes(A[i], d)
        S = S + y[i] * a
        Sm = Sm + abs(y[i]) * np.abs(a)
    return hc_mul64(Wp, S), hc_mul64(Wp, Sm, True), S


def prepare64(A, Cm, W, y, c_weight, d=0):
    """normsqrd, frob, trace as (value, magnitude): lmi_reference.prepare in float64."""
    n = A.shape[-1]
    WS, mWS, _ = weighted_slack64(A, Cm, W, y, c_weight, d)
    frob, frobm = np.trace(hc_mul64(WS, WS)[0]), np.trace(hc_mul64(mWS, mWS, True)[0])
    t, tm = np.trace(WS[0]), np.trace(mWS[0])
    return dict(normsqrd=(frob + 2 * t + n, frobm + 2 * tm + n), frob=(frob, frobm), trace=(-t, tm))


def take_step64(A, Cm, W, y, c_weight, e_weight, step, d=0):
    """lmi_reference.take_step restated in float64: (W_new, magnitude, growth); numpy.linalg.solve for the Pade
    system, growth = cond_1(V - U) (1 for the Taylor form of Hermitian data)."""
    n = A.shape[-1]
    WS, mWS, _ = weighted_slack64(A, Cm, W, y, c_weight, d)
    Wp = _planes(W, d)
    I = np.zeros_like(Wp)
    I[0] = np.eye(n)
    X = (WS + e_weight * I) * step
    mX = (mWS + abs(e_weight) * I) * abs(step)
    if d == 0:
        X2 = X[0] @ X[0]
        Um = X[0] @ (X2 + 60 * np.eye(n))
        V = 12 * X2 + 120 * np.eye(n)
        E = np.linalg.solve(V - Um, V + Um)[None]
        mE = np.abs(E) + hc_mul64(E, mX, True)
        growth = float(np.linalg.cond(V - Um, 1))
    else:
        F = I + X / 4 + hc_mul64(X, X / 4) / 8
        mF = I + mX / 4 + hc_mul64(mX, mX / 4, True) / 8
        F2 = hc_mul64(F, F)
        E = hc_mul64(F2, F2)
        mF2 = hc_mul64(mF, mF, True)
        mE = hc_mul64(mF2, mF2, True)
        growth = 1.0
    T = hc_mul64(E, Wp)
    Tm = hc_mul64(mE, Wp, True)
    Tt = np.swapaxes(T, -1, -2).copy()
    Tt[1:] = -Tt[1:]
    Wn = (T + Tt) / 2
    Wm = (Tm + np.swapaxes(Tm, -1, -2)) / 2
    return (Wn[0], Wm[0], growth) if d == 0 else (Wn, Wm, growth)


def pade_system64(A, Cm, W, y, c_weight, e_weight, step):
    """V - U of the real take step."""
    n = A.shape[-1]
    X = (W @ minus_s(A, Cm, y, c_weight) + e_weight * np.eye(n)) * step
    X2 = X @ X
    return 12 * X2 + 120 * np.eye(n) - X @ (X2 + 60 * np.eye(n))


kLuNB = 32  # the panel width of the Pade LU (kernels_lmi_large.hip.h)


def first_row_swap(M, columns=kLuNB):
    """The first column at which Gaussian elimination with partial pivoting (first largest |entry|) swaps rows, looking
    at the leading `columns` columns; None when it never does."""
    M = np.array(M, dtype=np.float64)
    for k in range(min(columns, M.shape[0] - 1)):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            return k
        f = M[k + 1:, k] / M[k, k]
        M[k + 1:, k + 1:] -= np.outer(f, M[k, k + 1:])
    return None


# The take steps past the old panel: minus_s = -KAPPA (I + rank two), X = (W minus_s + E_WEIGHT I) STEP.  With the
# eigenvalues of W log-spaced over [1e-6, 1] those of X run from -4 to 6, on both sides of the real root (4.64..) of
# the Pade denominator 120 - 60 x + 12 x^2 - x^3: V - U is indefinite with a diagonal around zero, and the partial
# pivoting swaps rows from the first columns on (within the first 32-column panel, the one lu_panel_tall factors).
E_WEIGHT, STEP, KAPPA = 6.0, 1.0, 10.0
# (order, seed, sparse route): 1024 / 1025 is the edge of the panel kernels; 1056 has a first panel of 1056 rows
# (lu_panel_tall) and a second of exactly 1024 (lu_panel<32>, every thread a row)
TALL_CASES = [(1024, 21, False), (1025, 22, False), (1056, 23, False), (1040, 24, True)]


def tall_case(n, seed, sparse):
    """(A, C, y, W) of a take step past the old panel: m = 2, W of condition 1e6.  Sparse route: diagonal A_i, the
    rank-two part in a dense C."""
    rng = np.random.default_rng(seed)
    if not sparse:
        A, Cm, y, _ = short_run_lmi(n, 2, RANK_TWO, seed)
        A, Cm = KAPPA * A, KAPPA * Cm
    else:
        Q = orthonormal(rng, n, 2)
        A = np.zeros((2, n, n))
        A[0] = np.diag(rng.uniform(-1, 1, n))
        A[1] = np.diag(rng.uniform(-1, 1, n))
        y = np.array([0.3, -0.2])
        Cm = KAPPA * (np.eye(n) + (Q * np.asarray(RANK_TWO)) @ Q.T) + np.tensordot(y, A, axes=1)
        Cm = 0.5 * (Cm + Cm.T)
    W = ref.ill_conditioned_W(rng, n, 1e6)
    swap = first_row_swap(pade_system64(A, Cm, W, y, C_WEIGHT, E_WEIGHT, STEP), kLuNB)
    assert swap is not None, "the partial pivoting of this Pade system swaps no rows within the first panel"
    return A, Cm, y, W


# ------------------------------------------------------------------ the long recurrences
# A run of n / 2 steps is determined by its input only while no Ritz value has converged: after that the
# unreorthogonalised vectors lose their biorthogonality and the other end of the spectrum turns into noise (which a
# generic slack reaches within some thirty steps).  Here W^1/2 minus_s W^1/2 has its n eigenvalues at the Chebyshev
# points of [-3, -0.2]: dense towards both ends, so that no Ritz value converges before step n and the whole run stays
# a smooth function of the data, at every length.
def long_spectrum(n):
    return -1.6 + 1.4 * np.cos(np.pi * (np.arange(n) + 0.5) / n)


def long_real_case(n, seed):
    """(prob, W, y) of one real constraint of order n (m = 4) at a well-conditioned scaling point; prob["A"] and
    prob["C"] carry a leading axis of one constraint, as the problems of conex_amd.synthetic do."""
    rng = np.random.default_rng(seed)
    W = syn.scaling_points(1, n, seed=seed + 5, scale=0.3)
    w, V = np.linalg.eigh(W[0])
    Wmh = (V / np.sqrt(w)) @ V.T
    Q = orthonormal(rng, n, n)
    T = Wmh @ ((Q * long_spectrum(n)) @ Q.T) @ Wmh
    T = 0.5 * (T + T.T)
    A = np.stack([syn.random_sym(rng, n) for _ in range(4)])
    y = rng.uniform(-1, 1, 4)
    Cm = np.tensordot(y, A, axes=1) - T
    return dict(A=A[None], C=Cm[None], n=n), W, y


def to_planes(Z):
    return np.stack([Z.real, Z.imag])


def long_complex_case(n, seed):
    """The same over C: planes (d = 2) of order n."""
    rng = np.random.default_rng(seed)
    H = ref.complex_rep(syn.random_hermitian(rng, 2, n), 2)
    Wc = np.eye(n) + 0.3 * H / np.linalg.norm(H, 2)  # (condition below 2)
    W = to_planes(0.5 * (Wc + Wc.conj().T))[None]
    w, V = np.linalg.eigh(ref.complex_rep(W[0], 2))
    Wmh = (V / np.sqrt(w)) @ V.conj().T
    Q = orthonormal(rng, n, n, complex_=True)
    T = Wmh @ ((Q * long_spectrum(n)) @ Q.conj().T) @ Wmh
    T = 0.5 * (T + T.conj().T)
    A = np.stack([syn.random_hermitian(rng, 2, n) for _ in range(4)])
    y = rng.uniform(-1, 1, 4)
    Cm = np.tensordot(y, A, axes=1) - to_planes(T)
    return dict(A=A[None], C=Cm[None], n=n), W, y


def long_real_determined(n, seed):
    """(query determined, PrepareStep determined, spectrum) by float64 alone (test_gpu_lmi_kernel_matrix.py,
    lanczos_determined)."""
    prob, W, y = long_real_case(n, seed)
    A, Cm = prob["A"][0], prob["C"][0]
    S = minus_s(A, Cm, y)
    WS = W[0] @ S
    lo, hi = ref.slack_spectrum(A, Cm, W[0], y, C_WEIGHT, 0)
    bar = STABLE * max(abs(lo), abs(hi))
    r_p, r_q = start_columns(WS, S)
    return (ref.ritz_spread(WS, W[0], r_q, n // 2) <= bar, ref.ritz_spread(WS, W[0], r_p, n // 2) <= bar, (lo, hi))


# ------------------------------------------------------------------ the end-to-end solve
def solve_case(n, seed=31):
    """max y_1 + y_2  s.t.  Q diag(C_1 - y_1 I, C_2 - y_2 I) Q' >= 0 with a random orthogonal Q (every matrix dense):
    (A (2, n, n), C, b, optimum = lambda_min(C_1) + lambda_min(C_2))."""
    rng = np.random.default_rng(seed)
    h = n // 2
    Q = orthonormal(rng, n, n)
    blocks = []
    for k in (h, n - h):
        R = syn.random_sym(rng, k)
        blocks.append(R / np.linalg.norm(R, 2))
    A = np.stack([Q[:, :h] @ Q[:, :h].T, Q[:, h:] @ Q[:, h:].T])
    Cm = Q[:, :h] @ blocks[0] @ Q[:, :h].T + Q[:, h:] @ blocks[1] @ Q[:, h:].T
    A = 0.5 * (A + np.swapaxes(A, -1, -2))
    Cm = 0.5 * (Cm + Cm.T)
    opt = float(np.linalg.eigvalsh(blocks[0])[0] + np.linalg.eigvalsh(blocks[1])[0])
    return A, Cm, np.ones(2), opt


def solve_dense_lmi(A, Cm, b):
    """One solve through conex.h (CONEX_AddDenseLMIConstraint) with the max-cut test's configuration: (solved, y)."""
    import ctypes as C

    import conex_api as ca
    L = ca.api()
    n, m = A.shape[-1], A.shape[0]
    cfg = ca.default_config()
    cfg.inv_sqrt_mu_max = 1000
    cfg.final_centering_steps = 4
    cfg.max_iterations = 100
    p = L.CONEX_CreateConeProgram()
    assert L.CONEX_SetNumberOfVariables(p, m) == 0
    a, c = ca.colmajor(A), ca.colmajor(Cm)
    assert L.CONEX_AddDenseLMIConstraint(p, ca.dp(a), n, n, m, ca.dp(c), n, n) == 0
    y = np.zeros(m)
    bb = np.ascontiguousarray(b, dtype=np.float64)
    ok = L.CONEX_Maximize(p, ca.dp(bb), m, C.byref(cfg), ca.dp(y), m)
    L.CONEX_DeleteConeProgram(p)
    return ok, y
