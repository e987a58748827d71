"""Kernel times of a quadratic cone whose matrix A is given by its nonzeros (kernels_quad_sparse.hip.h) against the
same cone with A dense, both on the streamed route.

  python tools/quad_sparse_speed.py                    # n = m - 1 in 256, 1024, 2048, 4096; dense Q and diagonal + rank 8
  python tools/quad_sparse_speed.py --n 1024 --q parts

One cone with a selection A (A1 = [I 0], A0 = e_m: the risk bound over n assets and the bound t).  Times come from the
library's kernel clocks (cxk_kernel_clock: hipEvent pairs around the launches of a stage): the median over the rounds
after warm-up.  The two forms are built in one process and their rounds alternate, so both see the same box in the
same state.  cxk_finalize is timed on the host around initialize(), once per form and shape (it includes the upload).
Prints one JSON line per shape and form of Q: microseconds per stage and form of A, their sum over assembly,
PrepareStep and TakeStep, and milliseconds of finalize.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("assembly", "query", "prepare", "take")
FORMS = ("sparse", "dense")


def problem(n, q_form, rank=8, seed=1):
    rng = np.random.default_rng(seed)
    m = n + 1
    D = rng.uniform(1.0, 2.0, n)
    F = rng.uniform(0.0, 1.0, (n, rank)) / np.sqrt(n)
    A = np.zeros((n + 1, m))
    A[1 + np.arange(n), np.arange(n)] = 1.0
    A[0, n] = 1.0
    c = 0.2 * rng.uniform(-1, 1, n + 1)
    c[0] = 1.0
    w = rng.uniform(-1, 1, n + 1)
    w[0] = 2.0 * np.sqrt(w[1:] @ (D * w[1:] + F @ (F.T @ w[1:])))
    y = rng.uniform(-1, 1, m) * 0.25
    S = (np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), D)
    return dict(n=n, m=m, q_form=q_form, S=S, F=F, D=D, A=A, c=c, W=w / w[0], y=y)


def csr_of(A):
    mask = A != 0
    rows, cols = np.nonzero(mask)
    return np.r_[0, np.cumsum(mask.sum(axis=1))].astype(np.int32), cols.astype(np.int32), A[rows, cols].copy()


def context(p, form):
    """form "sparse": A by its nonzeros; "dense": A as it is.  Q dense or by its parts in both.  (context, finalize ms)"""
    from conex_amd import KktContext
    k = KktContext(p["m"], device=0)
    k.set_streamed_quadratic(1)
    dense_q = p["q_form"] == "dense"
    Q = np.diag(p["D"]) + p["F"] @ p["F"].T if dense_q else None
    if form == "sparse":
        assert k.add_quadratic_csr(Q if dense_q else dict(S=p["S"], F=p["F"]), csr_of(p["A"]), p["c"]) == 0
    elif dense_q:
        assert k.add_quadratic(Q, p["A"], p["c"]) == 0
    else:
        assert k.add_quadratic_structured(p["S"], p["F"], None, p["A"], p["c"]) == 0
    t0 = time.perf_counter()
    k.initialize()
    k.sync()
    ms = (time.perf_counter() - t0) * 1e3
    assert k.count_streamed_quadratic() == 1 and k.count_sparse_quadratic() == (form == "sparse")
    k.set_W(0, p["W"])
    k.set_y(p["y"])
    k.enable_timing(True)
    return k, ms


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


def measure(p, rounds, warmup):
    out = {"n": p["n"], "m": p["m"], "q": p["q_form"], "nnz": int(np.count_nonzero(p["A"])), "rounds": rounds}
    ks = {}
    for form in FORMS:
        ks[form], out[f"finalize_{form}_ms"] = context(p, form)
        out[f"finalize_{form}_ms"] = round(out[f"finalize_{form}_ms"], 2)
    calls = {form: stage_calls(k, p["W"]) for form, k in ks.items()}
    times = {form: {s: [] for s in STAGES} for form in FORMS}
    for r in range(warmup + rounds):
        for form in FORMS:   # the forms alternate within a round
            for s in STAGES:
                us = once(ks[form], s, calls[form][s])
                if r >= warmup:
                    times[form][s].append(us)
    for form in FORMS:
        for s in STAGES:
            out[f"{s}_{form}_us"] = round(float(np.median(times[form][s])), 2)
        out[f"iteration_{form}_us"] = round(sum(out[f"{s}_{form}_us"] for s in ("assembly", "prepare", "take")), 2)
    for k in ks.values():
        k.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=0, help="one order (default: 256, 1024, 2048, 4096)")
    ap.add_argument("--q", choices=("dense", "parts", "both"), default="both")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    for n in ((a.n,) if a.n else (256, 1024, 2048, 4096)):
        for q in (("dense", "parts") if a.q == "both" else (a.q,)):
            print(json.dumps(measure(problem(n, q), a.rounds, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
