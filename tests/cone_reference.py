"""Extended-precision reference of the per-constraint stages of the cones that are not matrices
(numpy longdouble: a 64-bit mantissa on x86-64), from the formulas the oracle restates
(oracle/cxo_program.c, oracle/cxo_hermitian.c):

- linear (lin_*):  everything elementwise in w; G = A' diag(w^2) A, AW = A' w, AQc = A' (w^2 c),
  (sum w c, sum (w c)^2); d = w (A y - k c) + e; the query's w (A y - k c); the affine update
  w + w (w A y); the step w exp(t d); the line search's per-row interval of |d0 + t delta| <= dinf.
- second-order (soc_*) and quadratic (quad_*) cone: the spin factor with <x, y> = x0 y0 + x1' Q y1
  (Q = I for the second-order cone), Q(x) y = 2 <x, y> x - det(x) R y, det x = x0^2 - |x1|_Q^2,
  sqrt / exp through the two eigenvalues x0 +- |x1|_Q.  The second-order cone's Schur block goes
  through w^{1/2} (2 (Q(w^{1/2}) a_i)' (Q(w^{1/2}) a_j), Euclidean, as soc_schur forms it), the
  quadratic cone's is 2 <a_i, Q(w) a_j> written out in w itself (quad_schur).
- octonion cone (order <= 3): 8 planes, products through the sign table below (plane i ^ j takes
  sign[i][j] X_i Y_j), x o y = (x y + y x) / 2, Q(x) y = 2 x o (x o y) - (x o x) o y, the reference's
  heuristic step quantities and GeodesicUpdateScaled.
- constant block: a copy.

Every quantity is a pair (value, magnitude).  The magnitude is the same expression with every term
replaced by its absolute value (differences become sums, also under a square root) wherever the
inputs are the problem's exact data.  Where a stage works on quantities an earlier stage computed
(d, exp(t d), w^{1/2}), magnitudes are carried to FIRST ORDER, so that slack is not squared:

  a product:      M(a b) = |a| M(b) + M(a) |b| - |a| |b|      (= |a| |b| for exact factors)
  k = |x|_Q:      M(k) = M(x)' |Q| |x| / k                     (<= |M(x)|_2 for Q = I)
  a quotient:     M(a / b) = M(a) M(b) / b^2
  exp(a):         M = exp(a) (1 + M(a))

(the last as lmi_reference.take_step carries the rounding of its argument into the exponential).
|computed - exact| <= c u g M is then the bound of an honest float64 evaluation in any summation
order; g is the conditioning of the spectral square root at W, sqrt(lambda_max / lambda_min): the
cancellation in x0 - |x1| leaves w^{1/2} with an absolute error u lambda_max / sqrt(lambda_min),
g times its magnitude sqrt(lambda_max).  g = 1 for whatever does not go through w^{1/2}: the
linear cone, AW, the quadratic cone's Schur block, the octonion cone (its kernels never take a
square root of W) and the constant block.
"""
import numpy as np

LD = np.longdouble
U64 = 2.0 ** -53  # unit roundoff of float64

# The sign table of the hyper-complex product, as oracle/cxo_hermitian.c and kernels_oct.hip.h hold it.
OCT_SIGN = np.array([[1, 1, 1, 1, 1, 1, 1, 1], [1, -1, -1, 1, -1, 1, 1, -1], [1, 1, -1, -1, -1, -1, 1, 1],
                     [1, -1, 1, -1, -1, 1, -1, 1], [1, 1, 1, 1, -1, -1, -1, -1], [1, -1, 1, -1, 1, -1, 1, -1],
                     [1, -1, -1, 1, 1, -1, -1, 1], [1, 1, -1, -1, 1, 1, -1, -1]])


def ld(a):
    return np.asarray(a, dtype=LD)


# ------------------------------------------------------------------------------------ linear
def lin_slack(A, c, y, k):
    A, c, y = ld(A), ld(c), ld(y)
    return A @ y - c * LD(k), np.abs(A) @ np.abs(y) + np.abs(c) * abs(LD(k))


def lin_schur(A, c, w):
    A, c, w = ld(A), ld(c), ld(w)
    aA, w2 = np.abs(A), w * w
    wc = w * c
    return dict(G=((A * w2[:, None]).T @ A, (aA * w2[:, None]).T @ aA),
                AW=(A.T @ w, aA.T @ np.abs(w)),
                AQc=(A.T @ (w2 * c), aA.T @ (w2 * np.abs(c))),
                sc=(ld([np.sum(wc), np.sum(wc * wc)]), ld([np.sum(np.abs(wc)), np.sum(wc * wc)])), g=1.0)


def lin_prepare(A, c, w, y, c_weight, e_weight):
    w = ld(w)
    ms, msm = lin_slack(A, c, y, c_weight)
    d, dm = ms * w + LD(e_weight), msm * np.abs(w) + abs(LD(e_weight))
    return dict(d=(d, dm), normsqrd=(np.sum(d * d), np.sum(2 * np.abs(d) * dm - d * d)), norminfd=(np.max(np.abs(d)), np.max(dm)), g=1.0)


def lin_query(A, c, w, y, c_weight):
    w = ld(w)
    ms, msm = lin_slack(A, c, y, c_weight)
    ws, wsm = w * ms, np.abs(w) * msm
    return dict(lmin=(-np.max(ws), np.max(wsm)), lmax=(-np.min(ws), np.max(wsm)),
                frob=(np.sum(ws * ws), np.sum(2 * np.abs(ws) * wsm - ws * ws)), trace=(-np.sum(ws), np.sum(wsm)), g=1.0)


def lin_affine(A, c, w, y):
    """AffineUpdate: minus_s = A y (no c), W + W (W minus_s)."""
    w = ld(w)
    ms, msm = lin_slack(A, c, y, 0.0)
    return w + w * (ms * w), np.abs(w) + np.abs(w) * (msm * np.abs(w))


def lin_take(A, c, w, y, c_weight, e_weight, step):
    w = ld(w)
    d, dm = lin_prepare(A, c, w, y, c_weight, e_weight)["d"]
    t = LD(step)
    ex = np.exp(d * t)
    return w * ex, np.abs(w) * ex * (1 + dm * abs(t))


def lin_line_search(A, c, w, y0, y1, c_scaling, dinf):
    """Per row: d0 = 1 + w (A y0), delta = w (A y1 - c_s c) - w (A y0), the interval of t with
    |d0 + t delta| <= dinf.  Returns (lower ends, upper ends, delta)."""
    A, c, w = ld(A), ld(c), ld(w)
    d0 = (A @ ld(y0)) * w + 1
    d1 = (A @ ld(y1) - c * LD(c_scaling)) * w + 1
    delta = d1 - d0
    a, b = (LD(dinf) - d0) / delta, (-LD(dinf) - d0) / delta
    return np.minimum(a, b), np.maximum(a, b), delta


def line_search_result(lbs, ubs):
    """FindMinimumMu over all rows of all linear constraints: the upper end, -1 when the interval is empty."""
    lb, ub = max(np.max(l) for l in lbs), min(np.min(u) for u in ubs)
    return ub if lb <= ub else LD(-1)


# ------------------------------------------------------- spin factor: second-order / quadratic cone
def mulm(a, am, b, bm):
    """Magnitude of a product of two computed quantities, first order: |a| M(b) + M(a) |b| - |a| |b|
    (= |a| |b| for exact factors; M(a) M(b) would square the slack two magnitudes already carry)."""
    a, b = np.abs(a), np.abs(b)
    return a * bm + am * b - a * b


def _q(Q, x):
    return x if Q is None else ld(Q) @ x


def _qa(Q, xm):
    return xm if Q is None else np.abs(ld(Q)) @ xm


def qdot(Q, x, xm, y, ym):
    """x' Q y and its first-order magnitude  M(x)' |Q| |y| + |x|' |Q| M(y) - |x|' |Q| |y|."""
    ax, ay = np.abs(x), np.abs(y)
    return x @ _q(Q, y), xm @ _qa(Q, ay) + ax @ _qa(Q, ym) - ax @ _qa(Q, ay)


def qnorm(Q, x, xm):
    """k = |x|_Q = sqrt(x' Q x).  dk = x' Q dx / k, and the sum's own rounding is u |x|' |Q| |x| / (2 k):
    M(k) = M(x)' |Q| |x| / k, which is at most |M(x)|_2 for Q = I (a sum of squares cannot cancel)."""
    s = x @ _q(Q, x)
    k = np.sqrt(np.abs(s))
    sm = xm @ _qa(Q, np.abs(x))
    return k, (sm / k if k > 0 else np.sqrt(xm @ _qa(Q, xm)))


def spin_eigs(W, Q=None):
    W = ld(W)
    k, _ = qnorm(Q, W[1:], np.abs(W[1:]))
    return W[0] - k, W[0] + k


def spin_g(W, Q=None):
    lo, hi = spin_eigs(W, Q)
    return float(np.sqrt(hi / lo))


def spin_sqrt(W, Q=None):
    """w^{1/2} = ((f0 + f1) / 2, (f0 - f1) / 2 w1 / |w1|), f = sqrt(w0 +- |w1|), of an exact W.  The magnitude is
    the expression in absolute values, sqrt(|w0| + M(|w1|)) for both f: the factor g the bound carries is what
    the cancellation in w0 - |w1| adds to it."""
    W = ld(W)
    w1, w1m = W[1:], np.abs(W[1:])
    k, km = qnorm(Q, w1, w1m)
    f0, f1 = np.sqrt(W[0] + k), np.sqrt(W[0] - k)
    fm = np.sqrt(np.abs(W[0]) + km)
    z, zm = np.zeros_like(W), np.zeros_like(W)
    z[0], zm[0] = (f0 + f1) / 2, fm
    if k > 0:
        z[1:], zm[1:] = (f0 - f1) / 2 * w1 / k, fm * w1m * km / (k * k)
    return z, zm


def spin_exp(d, dm, Q=None):
    """exp(d) = (c, h d1), c = (f0 + f1) / 2, h = (f0 - f1) / (2 k), f = exp(d0 +- k), k = |d1|_Q.
    First order: df = f (d d0 +- dk), so M(f) = f (1 + M(d0) + M(k)); h is formed as a difference over k, so
    M(h) = (M(f0) + M(f1)) / (2 k) + h M(k) / k, and M(h d1_i) by the product rule."""
    k, km = qnorm(Q, d[1:], dm[1:])
    f0, f1 = np.exp(d[0] + k), np.exp(d[0] - k)
    fs = (f0 + f1) * (1 + dm[0] + km) / 2
    z, zm = np.zeros_like(d), np.zeros_like(d)
    z[0], zm[0] = (f0 + f1) / 2, fs
    if k > 0:
        h = (f0 - f1) / (2 * k)
        hm = fs / k + h * km / k
        z[1:], zm[1:] = h * d[1:], mulm(h, hm, d[1:], dm[1:])
    return z, zm


def spin_quadrep(x, xm, y, ym, Q=None):
    """Q(x) y = 2 <x, y> x - det(x) R y; y may hold several columns.  Magnitudes by the product rule."""
    ax, ay = np.abs(x), np.abs(y)
    n1, n1m = qdot(Q, x[1:], xm[1:], x[1:], xm[1:])
    det, detm = x[0] * x[0] - n1, mulm(x[0], xm[0], x[0], xm[0]) + n1m
    qx, qax, qxm = _q(Q, x[1:]), _qa(Q, ax[1:]), _qa(Q, xm[1:])
    xy = x[0] * y[0] + qx @ y[1:]
    xym = mulm(x[0], xm[0], y[0], ym[0]) + qxm @ ay[1:] + qax @ ym[1:] - qax @ ay[1:]
    sign = np.ones(len(x), dtype=LD)
    sign[0] = -1
    if y.ndim == 2:
        return (2 * np.outer(x, xy) + det * sign[:, None] * y,
                2 * mulm(x[:, None], xm[:, None], xy[None, :], xym[None, :]) + mulm(det, detm, y, ym))
    return 2 * xy * x + det * sign * y, 2 * mulm(xy, xym, x, xm) + mulm(det, detm, y, ym)


def spin_slack(A, c, y, k):
    return lin_slack(A, c, y, k)


def _gramm(X, Xm, Y, Ym):
    """Magnitude of X' Y (columns of computed quantities), product rule."""
    aX, aY = np.abs(X), np.abs(Y)
    return Xm.T @ aY + aX.T @ Ym - aX.T @ aY


def soc_schur(A, c, W):
    A, c, W = ld(A), ld(c), ld(W)
    ws, wsm = spin_sqrt(W)
    WA, WAm = spin_quadrep(ws, wsm, A, np.abs(A))
    wc, wcm = spin_quadrep(ws, wsm, c, np.abs(c))
    return dict(G=(2 * WA.T @ WA, 2 * _gramm(WA, WAm, WA, WAm)), AW=(2 * A.T @ W, 2 * np.abs(A).T @ np.abs(W)),
                AQc=(2 * WA.T @ wc, 2 * _gramm(WA, WAm, wc, wcm)),
                sc=(ld([2 * wc[0], 2 * wc @ wc]), ld([2 * wcm[0], 2 * _gramm(wc, wcm, wc, wcm)])), g=spin_g(W))


def _spin_d(A, c, W, y, c_weight, Q):
    ws, wsm = spin_sqrt(W, Q)
    ms, msm = spin_slack(A, c, y, c_weight)
    d, dm = spin_quadrep(ws, wsm, ms, msm, Q)
    return ws, wsm, d, dm


def _spin_ends(d, dm, Q):
    k, km = qnorm(Q, d[1:], dm[1:])
    return d[0] + k, d[0] - k, dm[0] + km


def _sumsq(e0, e1, em):
    return e0 * e0 + e1 * e1, mulm(e0, em, e0, em) + mulm(e1, em, e1, em)


def spin_prepare(A, c, W, y, c_weight, Q=None, quad=False):
    """PrepareStep of the second-order (Q None) and the quadratic cone: d = Q(w^{1/2}) minus_s + e,
    normsqrd = e0^2 + e1^2 (= 2 |d|^2), norminfd = max |e|, e = d0 +- |d1|; `wsqrt` is what the stage
    leaves in W: all of w^{1/2} for the second-order cone, its scalar part over the old W1 for the
    quadratic cone (the reference binds wsqrt_q0 to W0 itself)."""
    W = ld(W)
    ws, wsm, d, dm = _spin_d(A, c, W, y, c_weight, Q)
    d[0] += 1
    dm[0] += 1
    e0, e1, em = _spin_ends(d, dm, Q)
    left, leftm = (ws, wsm) if not quad else (np.r_[ws[:1], W[1:]], np.r_[wsm[:1], np.abs(W[1:])])
    return dict(d=(d, dm), normsqrd=_sumsq(e0, e1, em), norminfd=(max(abs(e0), abs(e1)), em),
                wsqrt=(left, leftm), g=spin_g(W, Q))


def spin_query(A, c, W, y, c_weight, Q=None):
    _, _, d, dm = _spin_d(A, c, W, y, c_weight, Q)
    e0, e1, em = _spin_ends(d, dm, Q)
    lmax, lmin = -min(e0, e1), -max(e0, e1)
    return dict(lmin=(lmin, em), lmax=(lmax, em), frob=_sumsq(e0, e1, em), trace=(lmax + lmin, 2 * em), g=spin_g(W, Q))


def spin_take(A, c, W, y, c_weight, step, Q=None):
    """W <- Q(w^{1/2}) exp(t d)."""
    ws, wsm, d, dm = _spin_d(A, c, ld(W), y, c_weight, Q)
    d[0] += 1
    dm[0] += 1
    t = LD(step)
    ex, exm = spin_exp(d * t, dm * abs(t), Q)
    return spin_quadrep(ws, wsm, ex, exm, Q)


def quad_schur(A, c, W, Q=None):
    """quad_schur's expressions: 2 <a_i, Q(w) a_j> in w itself (no square root: g = 1)."""
    A, c, W = ld(A), ld(c), ld(W)
    aA, ac, aW = np.abs(A), np.abs(c), np.abs(W)
    A0, A1, a0, a1 = A[0], A[1:], aA[0], aA[1:]
    qw, qwm = _q(Q, W[1:]), _qa(Q, aW[1:])
    qc, qcm = _q(Q, c[1:]), _qa(Q, ac[1:])
    det, detm = W[0] * W[0] - W[1:] @ qw, W[0] * W[0] + aW[1:] @ qwm
    scale, scalem = qw @ c[1:] + c[0] * W[0], qwm @ ac[1:] + ac[0] * aW[0]
    v, vm = A1.T @ qw + A0 * W[0], a1.T @ qwm + a0 * aW[0]
    gram = A1.T @ (A1 if Q is None else ld(Q) @ A1)
    gramm = a1.T @ (a1 if Q is None else np.abs(ld(Q)) @ a1)
    t, tm = np.outer(A0, A0) - gram, np.outer(a0, a0) + gramm
    G = 2 * (-det * t + 2 * np.outer(v, v))
    Gm = 2 * (mulm(det, detm, t, tm) + 2 * mulm(v[:, None], vm[:, None], v[None, :], vm[None, :]))
    r, rm = A1.T @ qc - A0 * c[0], a1.T @ qcm + a0 * ac[0]
    AQc = 2 * (det * r + 2 * v * scale)
    AQcm = 2 * (mulm(det, detm, r, rm) + 2 * mulm(v, vm, scale, scalem))
    z, zm = c[1:] @ qc - c[0] * c[0], ac[1:] @ qcm + c[0] * c[0]
    s1 = 2 * (det * z + 2 * scale * scale)
    s1m = 2 * (mulm(det, detm, z, zm) + 2 * mulm(scale, scalem, scale, scalem))
    return dict(G=(G, Gm), AW=(2 * v, 2 * vm), AQc=(AQc, AQcm), sc=(ld([2 * scale, s1]), ld([2 * scalem, s1m])), g=1.0)


# ------------------------------------------------------------------------------------ octonions
def oct_mul(X, Y, absolute=False):
    Z = np.zeros((8, X.shape[1], Y.shape[2]), dtype=LD)
    for i in range(8):
        for j in range(8):
            Z[i ^ j] += (np.abs(X[i]) @ np.abs(Y[j])) if absolute else OCT_SIGN[i, j] * (X[i] @ Y[j])
    return Z


def oct_jordan(X, Y, absolute=False):
    return (oct_mul(X, Y, absolute) + oct_mul(Y, X, absolute)) / 2


def oct_quadrep(X, Y, absolute=False):
    a = 2 * oct_jordan(X, oct_jordan(X, Y, absolute), absolute)
    b = oct_jordan(oct_jordan(X, X, absolute), Y, absolute)
    return a + b if absolute else a - b


def oct_qr(X, Xm, Y, Ym):
    """Q(X) Y of an exact X (Xm = |X|) and a computed Y: linear in Y."""
    return oct_quadrep(X, Y), oct_quadrep(Xm, Ym, True)


def _oct_tabs(X1, X2, Y):
    """|.|-version of the polarised map  X1 o (X2 o Y) + X2 o (X1 o Y) - (X1 o X2) o Y  (= Q(X) Y at X1 = X2 = X)."""
    J = lambda a, b: oct_jordan(a, b, True)  # noqa: E731
    return J(X1, J(X2, Y)) + J(X2, J(X1, Y)) + J(J(X1, X2), Y)


def oct_qr_of_computed(S, Sm, W):
    """Q(S) W of a computed S and an exact W, first order: one factor S at a time carries its magnitude."""
    aS = np.abs(S)
    return oct_quadrep(S, W), 2 * _oct_tabs(Sm, aS, np.abs(W)) - _oct_tabs(aS, aS, np.abs(W))


def oct_herm(X, absolute=False):
    T = np.swapaxes(X, -1, -2).copy()
    if not absolute:
        T[1:] = -T[1:]
    return (X + T) / 2


def oct_schur(A, C, W):
    """A: (m, 8, n, n) planes, C, W: (8, n, n)."""
    A, C, W = ld(A), ld(C), ld(W)
    aA, aC, aW = np.abs(A), np.abs(C), np.abs(W)
    m = A.shape[0]
    QA = [oct_qr(W, aW, A[i], aA[i]) for i in range(m)]
    G = ld([[np.sum(A[j] * QA[i][0]) for i in range(m)] for j in range(m)])
    Gm = ld([[np.sum(aA[j] * QA[i][1]) for i in range(m)] for j in range(m)])
    QC, QCm = oct_qr(W, aW, C, aC)
    return dict(G=(G, Gm), AW=(ld([np.sum(A[i] * W) for i in range(m)]), ld([np.sum(aA[i] * aW) for i in range(m)])),
                AQc=(ld([np.sum(C * QA[i][0]) for i in range(m)]), ld([np.sum(aC * QA[i][1]) for i in range(m)])),
                sc=(ld([np.sum(C * W), np.sum(C * QC)]), ld([np.sum(aC * aW), np.sum(aC * QCm)])), g=1.0)


def oct_slack(A, C, y, k):
    A, C, y = ld(A), ld(C), ld(y)
    return np.tensordot(y, A, axes=1) - LD(k) * C, np.tensordot(np.abs(y), np.abs(A), axes=1) + abs(LD(k)) * np.abs(C)


def _oct_sums(A, C, W, y, c_weight):
    W = ld(W)
    S, Sm = oct_slack(A, C, y, c_weight)
    QS, QSm = oct_qr(W, np.abs(W), S, Sm)
    return (np.sum(W * S), np.sum(np.abs(W) * Sm)), (np.sum(QS * S), np.sum(mulm(QS, QSm, S, Sm)))


def oct_prepare(A, C, W, y, c_weight):
    """The reference's heuristic rules: normsqrd = <Q(W) s, s> + 2 <W, s> + n, norminfd = (<W, s> + n) / 3."""
    n = np.shape(W)[-1]
    (t, tm), (q, qm) = _oct_sums(A, C, W, y, c_weight)
    return dict(normsqrd=(q + 2 * t + n, qm + 2 * tm + n), norminfd=((t + n) / 3, (tm + n) / 3), g=1.0)


def oct_query(A, C, W, y, c_weight):
    (t, tm), (q, qm) = _oct_sums(A, C, W, y, c_weight)
    den, denm = LD(1e-15) + abs(t), LD(1e-15) + tm
    lmax, lmaxm = abs(q) / den, qm * denm / (den * den)
    return dict(lmin=(lmax / 100, lmaxm / 100), lmax=(lmax, lmaxm), frob=(q, qm), trace=(-t, tm), g=1.0)


def oct_take(A, C, W, y, c_weight, step):
    """GeodesicUpdateScaled: herm(c^2 W + 2 c k Q(W) s + k^2 Q(W) (Q(s) W)), c = 1.5, k = 0.5, s = t minus_s."""
    W = ld(W)
    aW = np.abs(W)
    S, Sm = oct_slack(A, C, y, c_weight)
    S, Sm = S * LD(step), Sm * abs(LD(step))
    q1, q1m = oct_qr(W, aW, S, Sm)
    q2, q2m = oct_qr_of_computed(S, Sm, W)
    q3, q3m = oct_qr(W, aW, q2, q2m)
    return oct_herm(W * LD(2.25) + q1 * LD(1.5) + q3 * LD(0.25)), oct_herm(aW * LD(2.25) + q1m * LD(1.5) + q3m * LD(0.25), True)


# ------------------------------------------------------------------------------- constant block
def static_schur(G, AQc0=None):
    G = np.asarray(G, dtype=np.float64)
    m = G.shape[0]
    return dict(G=G.copy(), AW=np.zeros(m), AQc=np.zeros(m) if AQc0 is None else np.asarray(AQc0, dtype=np.float64).copy(),
                sc=np.zeros(2))


# ------------------------------------------------------------------------------- scaling points
def lin_scaling_point(rng, r, cond):
    """Entries log-uniform over `cond`, the largest exactly 1 (cond "well": the suite's usual [0.5, 1.5] scaled)."""
    w = rng.uniform(0.5, 1.5, r) if cond == "well" else np.exp(-rng.uniform(0, np.log(cond), r))
    return w / np.max(w)


def spin_scaling_point(rng, n, cond, Q=None):
    """(w0, w1) with lambda_max = w0 + |w1|_Q = 1: "well" as the suite's usual points (|w1| <= 0.3 sqrt(n) ahead of a
    margin in [0.5, 1.5]); else lambda_min = 1 / cond along a random direction of unit Q-norm."""
    v = rng.standard_normal(n)
    Qm = np.eye(n) if Q is None else np.asarray(Q)
    if cond == "well":
        w1 = rng.uniform(-0.3, 0.3, n)
        w = np.r_[np.sqrt(w1 @ Qm @ w1) + rng.uniform(0.5, 1.5), w1]
        return w / (w[0] + np.sqrt(w1 @ Qm @ w1))
    v /= np.sqrt(v @ Qm @ v)
    return np.r_[(1 + 1 / cond) / 2, (1 - 1 / cond) / 2 * v]


def conditioned_Q(rng, n, cond):
    """Symmetric positive definite, eigenvalues log-spaced from 1 down to 1 / cond."""
    V, R = np.linalg.qr(rng.standard_normal((n, n)))
    Q = (V * np.logspace(0.0, -np.log10(cond), n)) @ V.T
    return 0.5 * (Q + Q.T)


def oct_random_hermitian(rng, n):
    R = rng.uniform(-1.0, 1.0, (8, n, n))
    H = np.empty_like(R)
    H[0] = R[0] + R[0].T
    for p in range(1, 8):
        H[p] = R[p] - R[p].T
    return H


def oct_scaling_point(rng, n, cond):
    """Q(H) D, H = I + a small Hermitian matrix (Q(H) maps the cone onto itself), D real diagonal: ones at "well",
    else log-spaced from 1 down to 1 / cond; scaled to the largest diagonal entry 1."""
    H = oct_random_hermitian(rng, n) * 0.1
    H[0] += np.eye(n)
    D = np.zeros((8, n, n))
    D[0] = np.diag(np.ones(n) if cond == "well" else np.logspace(0.0, -np.log10(cond), n))
    W = np.asarray(oct_herm(oct_quadrep(ld(H), ld(D))), dtype=np.float64)
    return W / np.max(np.diag(W[0]))
