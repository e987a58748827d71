"""Kernel times of the streamed quadratic cone path (kernels_quad_stream.hip.h) against the LDS route.

  python tools/quad_stream_speed.py --cones 1 --n 2000 --m 2000 --q      # a risk constraint over 2000 assets
  python tools/quad_stream_speed.py --cones 1 --n 20000 --m 8            # beyond LDS: the streamed route only
  python tools/quad_stream_speed.py --cones 64 --n 256 --m 16 --q        # a batch
  python tools/quad_stream_speed.py --sweep                              # the threshold sweep (one cone, Q, m = 8)

Times come from the library's kernel clocks (cxk_kernel_clock: hipEvent pairs around the launches of a stage): the
median over the rounds after warm-up.  Where the LDS route admits the shape, both routes are built in the same process
(cxk_set_streamed_quadratic 1 and 0) and their rounds alternate, so both see the same box in the same state.  Prints
one JSON line per shape: microseconds per stage and route, and the streamed stage's share of its HBM bound,
passes * 8 n^2 + 8 (n + 1) m bytes at the data sheet's 8 TB/s (passes over Q: assembly 1, query 2, PrepareStep 2,
TakeStep 0).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12         # bytes/s, MI355X data sheet
LDS_DOUBLES = (160 * 1024 - 512) // 8
PASSES = {"assembly": 1, "query": 2, "prepare": 2, "take": 0}
STAGES = ("assembly", "query", "prepare", "take")


def lds_route(n, m):
    return m + 4 * (n + 1) <= LDS_DOUBLES and 2 * n + m + 4 <= LDS_DOUBLES and 3 * (n + 1) <= LDS_DOUBLES


def context(cones, n, m, with_q, mode):
    from conex_amd import KktContext, synthetic as syn
    rng = np.random.default_rng(1)
    cliques, num_vars = syn.chain_cliques(cones, m, 1 if m > 1 else 0)
    k = KktContext(num_vars, device=0)
    k.set_streamed_quadratic(mode)
    W = []
    for cl in cliques:
        A = rng.uniform(-1, 1, (n + 1, m))
        c = 0.2 * rng.uniform(-1, 1, n + 1)
        c[0] = 1.0
        Q = None
        if with_q:
            R = rng.uniform(-1, 1, (n, n))
            Q = R @ R.T / n + np.eye(n)
        assert k.add_quadratic(Q, A, c, cl) >= 0
        w = rng.uniform(-1, 1, n + 1)
        w[0] = 2.0 * np.sqrt(w[1:] @ (Q @ w[1:] if with_q else w[1:]))
        W.append(w / w[0])
    k.initialize()
    assert k.count_streamed_quadratic() == (cones if mode else 0)
    for i, w in enumerate(W):
        k.set_W(i, w)
    y = rng.uniform(-1, 1, k.N)
    y *= 0.25 / (m * 1.0)
    k.set_y(y)
    k.enable_timing(True)
    return k, W


def stage_calls(k, W):
    def prepare():   # (PrepareStep leaves the scalar part of w^{1/2} in W0: the same W every round)
        for i, w in enumerate(W):
            k.set_W(i, w)
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


def measure(cones, n, m, with_q, rounds, warmup, lds_rounds):
    out = {"cones": cones, "n": n, "m": m, "Q": bool(with_q), "rounds": rounds}
    routes = {"streamed": context(cones, n, m, with_q, 1)}
    if lds_route(n, m) and lds_rounds > 0:
        routes["lds"] = context(cones, n, m, with_q, 0)
        out["lds_rounds"] = min(rounds, lds_rounds)
    calls = {name: stage_calls(k, W) for name, (k, W) in routes.items()}
    times = {name: {s: [] for s in STAGES} for name in routes}
    for r in range(warmup + rounds):
        for name, (k, _) in routes.items():   # the routes alternate within a round
            if name == "lds" and r >= min(warmup, lds_rounds) + min(rounds, lds_rounds):
                continue
            for s in STAGES:
                us = once(k, s, calls[name][s])
                if r >= (warmup if name == "streamed" else min(warmup, lds_rounds)):
                    times[name][s].append(us)
    for name in routes:
        for s in STAGES:
            out[f"{s}_{name}_us"] = round(float(np.median(times[name][s])), 2)
    for s in STAGES:
        bytes_ = cones * (PASSES[s] * 8.0 * n * n * (1 if with_q else 0) + 8.0 * (n + 1) * m)
        out[f"{s}_share_of_hbm_bound"] = round(bytes_ / HBM_PEAK / (out[f"{s}_streamed_us"] * 1e-6), 4)
    for name in routes:
        out[f"iteration_{name}_us"] = round(sum(out[f"{s}_{name}_us"] for s in ("assembly", "prepare", "take")), 2)
    for k, _ in routes.values():
        k.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cones", type=int, default=1)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--m", type=int, default=2000)
    ap.add_argument("--q", action="store_true", help="the cones carry a dense inner-product matrix Q")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lds-rounds", type=int, default=30,
                    help="rounds of the LDS route (its one-thread products take seconds at large n); 0 leaves it out")
    ap.add_argument("--sweep", action="store_true", help="n in 32 .. 1024 with Q, m = 8, one cone: the threshold sweep")
    a = ap.parse_args()
    if a.sweep:
        for n in (32, 64, 128, 256, 512, 1024):
            print(json.dumps(measure(1, n, 8, True, a.rounds, a.warmup, a.lds_rounds)), flush=True)
    else:
        print(json.dumps(measure(a.cones, a.n, a.m, a.q, a.rounds, a.warmup, a.lds_rounds)), flush=True)


if __name__ == "__main__":
    main()
