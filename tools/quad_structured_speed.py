"""Kernel times of quadratic cones whose Q = S + F diag(sigma) F' is given by its parts (kernels_quad_structured.hip.h)
against the dense streamed route on the expanded Q.

  python tools/quad_structured_speed.py --compare     # n in 256 .. 16384: structured against dense streamed
  python tools/quad_structured_speed.py --large       # structured alone at n = 1e5 and 1e6
  python tools/quad_structured_speed.py --lanes       # nnz/row in 3 .. 243 at n = 16384 under each CXK_QUAD_CSR_LANES
  python tools/quad_structured_speed.py --n 4096 --band 1 --rank 8

One cone, m = 8, S a band matrix (--band sub-diagonals: 1 is tridiagonal) plus rank 8 unless said otherwise.  Times come
from the library's kernel clocks (cxk_kernel_clock: hipEvent pairs around the launches of a stage): the median over the
rounds after warm-up.  The routes (or the lane counts) are built in one process and their rounds alternate, so all see
the same box in the same state.  Prints one JSON line per shape: microseconds per stage and route, and the structured
stage's share of its byte bound, passes * (12 nnz + 16 n rank) + 8 (n + 1) m bytes at the data sheet's 8 TB/s (F is read
by the dots and by the rows; passes over Q: assembly 1, query 2, PrepareStep 2, TakeStep 0).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12         # bytes/s, MI355X data sheet
PASSES = {"assembly": 1, "query": 2, "prepare": 2, "take": 0}
STAGES = ("assembly", "query", "prepare", "take")
LANES = (1, 8, 64)


def banded(rng, n, width):
    """(indptr, indices, data) of a symmetric band matrix with `width` sub-diagonals, strictly diagonally dominant."""
    width = min(width, n - 1)
    idx, val = [np.stack([np.arange(n), np.arange(n)])], [rng.uniform(2.0, 3.0, n)]
    for k in range(1, width + 1):
        o = rng.uniform(0.0, 1.0, n - k) / (2.0 * width)
        r = np.arange(n - k)
        idx += [np.stack([r + k, r]), np.stack([r, r + k])]
        val += [o, o]
    rc, v = np.concatenate(idx, axis=1), np.concatenate(val)
    order = np.lexsort((rc[1], rc[0]))
    rows, cols, v = rc[0][order], rc[1][order], v[order]
    indptr = np.r_[0, np.cumsum(np.bincount(rows, minlength=n))].astype(np.int32)
    return indptr, cols.astype(np.int32), v


def apply_q(S, F, x):
    indptr, indices, data = S
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    return np.bincount(rows, weights=data * x[indices], minlength=len(x)) + F @ (F.T @ x)


def problem(n, m, band, rank, seed=1):
    rng = np.random.default_rng(seed)
    S = banded(rng, n, band)
    F = rng.uniform(0.0, 1.0, (n, rank)) / np.sqrt(n)
    A = rng.uniform(-1, 1, (n + 1, m))
    c = 0.2 * rng.uniform(-1, 1, n + 1)
    c[0] = 1.0
    w = rng.uniform(-1, 1, n + 1)
    w[0] = 2.0 * np.sqrt(w[1:] @ apply_q(S, F, w[1:]))
    y = rng.uniform(-1, 1, m) * 0.25 / m
    return dict(n=n, m=m, S=S, F=F, A=A, c=c, W=w / w[0], y=y)


def context(p, route, lanes=None):
    """route "structured": by the parts; "dense": the expanded Q on the streamed route."""
    from conex_amd import KktContext
    k = KktContext(p["m"], device=0)
    if route == "structured":
        if lanes:
            os.environ["CXK_QUAD_CSR_LANES"] = str(lanes)
        else:
            os.environ.pop("CXK_QUAD_CSR_LANES", None)
        assert k.add_quadratic_structured(p["S"], p["F"], None, p["A"], p["c"]) == 0
    else:
        k.set_streamed_quadratic(1)
        n = p["n"]
        indptr, indices, data = p["S"]
        Q = p["F"] @ p["F"].T
        Q[np.repeat(np.arange(n), np.diff(indptr)), indices] += data
        assert k.add_quadratic(Q, p["A"], p["c"]) == 0
        del Q
    k.initialize()  # (the lane count is read here)
    os.environ.pop("CXK_QUAD_CSR_LANES", None)
    assert k.count_streamed_quadratic() == 1 and k.count_structured_quadratic() == (route == "structured")
    k.set_W(0, p["W"])
    k.set_y(p["y"])
    k.enable_timing(True)
    return k


def stage_calls(k, W):
    def prepare():   # (PrepareStep leaves the scalar part of w^{1/2} in W0: the same W every round)
        k.set_W(0, W)
        k.prepare_step(None, 1.0, 1.0)

    def take():
        prepare()
        k.take_step(0.5, 1.0)

    return {"assembly": k.assemble, "query": lambda: k.weighted_slack_eigenvalues(None, 1.0), "prepare": prepare, "take": take}


def once(k, slot, call):
    """One call of a stage: microseconds of its clock slot."""
    for s in STAGES:
        k.kernel_clock(s, reset=True)
    call()
    k.sync()
    n, ms = k.kernel_clock(slot, reset=True)
    assert n == 1, (slot, n)
    return ms * 1e3


def measure(p, names, rounds, warmup, band, rank):
    """`names`: the contexts of one process, "dense", "structured" or "lanes-L"."""
    nnz = int(p["S"][0][-1])
    out = {"n": p["n"], "m": p["m"], "nnz_per_row": round(nnz / p["n"], 2), "band": band, "rank": rank, "rounds": rounds}
    ks = {}
    for name in names:
        ks[name] = context(p, "dense" if name == "dense" else "structured", int(name[6:]) if name.startswith("lanes-") else None)
    calls = {name: stage_calls(k, p["W"]) for name, k in ks.items()}
    times = {name: {s: [] for s in STAGES} for name in names}
    for r in range(warmup + rounds):
        for name in names:   # the contexts alternate within a round
            for s in STAGES:
                us = once(ks[name], s, calls[name][s])
                if r >= warmup:
                    times[name][s].append(us)
    for name in names:
        for s in STAGES:
            out[f"{s}_{name}_us"] = round(float(np.median(times[name][s])), 2)
        out[f"iteration_{name}_us"] = round(sum(out[f"{s}_{name}_us"] for s in ("assembly", "prepare", "take")), 2)
    first = next(nm for nm in names if nm != "dense")
    for s in STAGES:
        bytes_ = PASSES[s] * (12.0 * nnz + 16.0 * p["n"] * rank) + 8.0 * (p["n"] + 1) * p["m"]
        out[f"{s}_share_of_byte_bound"] = round(bytes_ / HBM_PEAK / (out[f"{s}_{first}_us"] * 1e-6), 4)
    for k in ks.values():
        k.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--m", type=int, default=8)
    ap.add_argument("--band", type=int, default=1, help="sub-diagonals of S (1: tridiagonal, 3 nonzeros per row)")
    ap.add_argument("--rank", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--compare", action="store_true", help="n in 256 .. 16384: structured against dense streamed")
    ap.add_argument("--max-dense-n", type=int, default=16384, help="largest n of --compare (the expansion is 8 n^2 bytes, four times on the host)")
    ap.add_argument("--large", action="store_true", help="structured alone at n = 1e5 and 1e6")
    ap.add_argument("--lanes", action="store_true", help="nnz/row in 3 .. 243 at n = 16384 under each lane count")
    a = ap.parse_args()

    def emit(p, names, band):
        print(json.dumps(measure(p, names, a.rounds, a.warmup, band, a.rank)), flush=True)

    if a.compare:
        for n in (256, 1024, 4096, 16384):
            if n <= a.max_dense_n:
                emit(problem(n, a.m, 1, a.rank), ("structured", "dense"), 1)
    if a.large:
        for n in (100_000, 1_000_000):
            emit(problem(n, a.m, 1, a.rank), ("structured",), 1)
    if a.lanes:
        for band in (1, 4, 13, 40, 121):   # 3, 9, 27, 81, 243 nonzeros per row
            emit(problem(16384, a.m, band, a.rank), tuple(f"lanes-{L}" for L in LANES), band)
    if not (a.compare or a.large or a.lanes):
        emit(problem(a.n, a.m, a.band, a.rank), ("structured",), a.band)


if __name__ == "__main__":
    main()
