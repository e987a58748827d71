"""lmi_schur_mfma walks each workgroup's constraints first to last in one launch of a group and last to
first in the next (cone_lmi.hip, LaunchLmiDenseSchur; CXK_LMI_ORDER=forward keeps the one order).  The order
may change nothing but the time: every constraint's G, AW, AQc and scalars are the same bits in both.

Each case runs four consecutive assemblies on one context (orders forward, backward, forward, backward), at a
different scaling point W before each, so that a constraint the launch skipped or wrote to another
constraint's slot cannot hide behind what the launch before it left there.  After each launch every
constraint's blocks and the scattered residuals are compared, byte for byte, with a fresh context's first
launch at that W (always forward) and with the same sequence on a context created under
CXK_LMI_ORDER=forward, and a sample of constraints with the CPU oracle at the suite's 1e-13.

Shapes: the smallest at which the order can go wrong, on a device of 256 CUs (256 workgroups) --
workgroups with 2 and 1 constraints (K = 257), with 3 and 2 (K = 513), the flagship instance with two P
images and the one-image form (whose producers and consumers take turns), the folded Hermitian instance, and
K = 200, where every workgroup has one constraint and both orders are the same launch.
"""
import numpy as np
import pytest

import oracle_lib as ol
from conex_amd import KktContext
from conex_amd import synthetic as syn

pytestmark = pytest.mark.gpu

TOL_SCHUR = 1e-13  # tests/test_gpu_parity.py
LAUNCHES = 4

# (id, kind, K, n, m, d, the Schur instance every constraint must report)
CASES = [
    ("k257-n8-m3", "lmi", 257, 8, 3, 0, "lmi_schur_mfma<8> exact two-images"),
    ("k513-n12-m5", "lmi", 513, 12, 5, 0, "lmi_schur_mfma<12> exact two-images"),
    ("k300-n20-m20", "lmi", 300, 20, 20, 0, "lmi_schur_mfma<20> exact two-images"),
    ("k300-n20-m23-one-image", "lmi", 300, 20, 23, 0, "lmi_schur_mfma<20> exact one-image"),
    ("k260-c12-m24-folded", "herm", 260, 12, 24, 2, "lmi_schur_mfma<24,folded> two-images"),
    ("k200-n20-m20", "lmi", 200, 20, 20, 0, "lmi_schur_mfma<20> exact two-images"),
]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = np.linalg.norm(b)
    return np.linalg.norm(a - b) / n if n > 0 else np.linalg.norm(a - b)


def problem(kind, K, n, m, d, seed):
    overlap = max(1, min(3, m // 3))
    if kind == "herm":
        prob = syn.hermitian_problem(K=K, n=n, d=d, m=m, branching=4, overlap=overlap, seed=seed)
        Ws = [syn.hermitian_scaling_points(K, n, d, seed=seed + 11 + j) for j in range(LAUNCHES)]
    else:
        prob = syn.lmi_problem(K=K, n=n, m=m, branching=4, overlap=overlap, seed=seed)
        Ws = [syn.scaling_points(K, n, seed=seed + 11 + j) for j in range(LAUNCHES)]
    return prob, Ws


def set_points(ctx, W):
    for i in range(ctx.K):
        ctx.set_W(i, W[i])


def snapshot(k):
    """What one assembly wrote: per constraint (lower triangle of G, AW, AQc, scalars), then the residuals."""
    out = []
    for i in range(k.K):
        G, AW, AQc, sc = k.constraint_schur(i)
        out.append((np.tril(G), AW, AQc, sc))
    return out, k.residuals()


def first_difference(a, b):
    """None if two snapshots hold the same bytes, else where they first differ."""
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        for name, u, v in zip(("G", "AW", "AQc", "scalars"), x, y):
            if u.tobytes() != v.tobytes():
                return f"{name} of constraint {i}"
    for name, u, v in zip(("AW", "AQc", "scalars"), a[1], b[1]):
        if u.tobytes() != v.tobytes():
            return f"residual {name}"
    return None


def sample(K):
    return sorted({0, 1, 199, 200, 255, 256, 257, K // 2, K - 2, K - 1} & set(range(K)))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_alternating_order_writes_the_same_bits(case, monkeypatch):
    cid, kind, K, n, m, d, instance = case
    prob, Ws = problem(kind, K, n, m, d, seed=4000 + K + n)
    monkeypatch.delenv("CXK_LMI_ORDER", raising=False)
    alt = syn.build(KktContext, prob, kind, device=0)
    monkeypatch.setenv("CXK_LMI_ORDER", "forward")
    fwd = syn.build(KktContext, prob, kind, device=0)
    monkeypatch.delenv("CXK_LMI_ORDER")
    for i in sample(K):
        assert alt.lmi_kernels(i)["schur"] == instance
    o = syn.build(ol.Program, prob, kind)
    for j, W in enumerate(Ws):
        fresh = syn.build(KktContext, prob, kind, device=0)
        snaps = []
        for ctx in (alt, fwd, fresh):
            set_points(ctx, W)
            ctx.assemble()
            snaps.append(snapshot(ctx))
        del fresh
        where = first_difference(snaps[0], snaps[2])
        assert where is None, f"launch {j}: {where} differs from a fresh context's first launch"
        where = first_difference(snaps[0], snaps[1])
        assert where is None, f"launch {j}: {where} differs from the forward order"
        set_points(o, W)
        o.assemble()
        for i in sample(K):
            Go, AWo, AQo, sco = o.constraint_schur(i)
            Gk, AWk, AQk, sck = snaps[0][0][i]
            assert rel(Gk, np.tril(Go)) <= TOL_SCHUR, (j, i)
            assert rel(AWk, AWo) <= TOL_SCHUR and rel(AQk, AQo) <= TOL_SCHUR and rel(sck, sco) <= TOL_SCHUR, (j, i)


def test_kkt_solve_in_both_parities(monkeypatch):
    """Assembly and tree launch together: the same four solves with the launch orders forward, backward, ...
    (a new context), backward, forward, ... (one assembly ahead) and forward throughout give the same y."""
    K, n, m = 300, 20, 20
    prob, Ws = problem("lmi", K, n, m, 0, seed=4700)
    monkeypatch.delenv("CXK_LMI_ORDER", raising=False)
    even = syn.build(KktContext, prob, "lmi", device=0)
    odd = syn.build(KktContext, prob, "lmi", device=0)
    monkeypatch.setenv("CXK_LMI_ORDER", "forward")
    fwd = syn.build(KktContext, prob, "lmi", device=0)
    monkeypatch.delenv("CXK_LMI_ORDER")
    set_points(odd, Ws[-1])
    odd.assemble()
    for j, W in enumerate(Ws):
        ys = []
        for ctx in (even, odd, fwd):
            set_points(ctx, W)
            ok, y = ctx.kkt_solve(prob["b"], 0.7, 0.9, 0.8)
            assert ok == 1
            ys.append(y)
        assert ys[0].tobytes() == ys[1].tobytes(), f"solve {j}: y differs between the two parities"
        assert ys[0].tobytes() == ys[2].tobytes(), f"solve {j}: y differs from the forward order"
