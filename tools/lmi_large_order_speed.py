"""Kernel times of the large-order matrix-inequality route at and past its old one-workgroup limits: the Lanczos run
behind the eigenvalue query and PrepareStep on one workgroup (lmi_large_spectrum) against the chip-wide run
(kernels_lmi_wide.hip.h), and TakeStep across the 1024-row edge of the Pade LU's panel kernels.

  python tools/lmi_large_order_speed.py                      # the three tables of DESIGN.md 4.5.6
  python tools/lmi_large_order_speed.py --spectrum 512       # one order, both runs
  python tools/lmi_large_order_speed.py --wide-only 4000     # beyond 2549: the chip-wide run alone
  python tools/lmi_large_order_speed.py --take 2048          # TakeStep
  python tools/lmi_large_order_speed.py --short 2550         # a run that breaks after three steps: its empty launches

Times come from the library's kernel clocks (cxk_kernel_clock: hipEvent pairs around the launches of a stage): the
median over the rounds after warm-up.  Both runs are built in the same process (cxk_set_wide_spectrum 0 and 1) and
their rounds alternate.  One real constraint, m = 1, W = I; the slack has its n eigenvalues at the Chebyshev points of
[-3, -0.2], so that no Ritz value converges and the recurrence runs its full n / 2 steps (the worst case; a solve's
runs usually break earlier).  --short: slack identity plus rank two, the run breaks at step 3 and the remaining
launches return at once; what one such launch costs is the stage time over their number.
From --slow-from on the one-workgroup run takes seconds per call: it gets --slow-rounds rounds and no warm-up.

The share of the panel kernels in TakeStep is not a clock of the library: run
  rocprofv3 --kernel-trace --stats -- python tools/lmi_large_order_speed.py --take 2048 --rounds 5
and divide the lu_panel / lu_panel_tall rows of the kernel statistics by the sum of the TakeStep kernels.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPECTRUM_ORDERS = (256, 512, 1000, 2000, 2549)
WIDE_ONLY_ORDERS = (2560, 4000)
TAKE_ORDERS = (1024, 1025, 2048, 4000)
MAX_ONE_WORKGROUP = 2549


def orthonormal(rng, n, k):
    return np.linalg.qr(rng.standard_normal((n, k)))[0]


def long_slack(n, rng):
    """minus_s with its eigenvalues at the Chebyshev points of [-3, -0.2]."""
    lam = -1.6 + 1.4 * np.cos(np.pi * (np.arange(n) + 0.5) / n)
    Q = orthonormal(rng, n, n)
    T = (Q * lam) @ Q.T
    return 0.5 * (T + T.T)


def short_slack(n, rng):
    """minus_s = -(I + 0.7 u u' - 0.4 v v')."""
    Q = orthonormal(rng, n, 2)
    T = -(np.eye(n) + (Q * np.array([0.7, -0.4])) @ Q.T)
    return 0.5 * (T + T.T)


def context(n, minus_s, mode):
    from conex_amd import KktContext
    k = KktContext(1, device=0)
    k.set_wide_spectrum(mode)
    R = np.random.default_rng(2).uniform(-1, 1, (n, n))
    assert k.add_lmi(0.5 * (R + R.T)[None], -minus_s) == 0  # a dense A_1 (the dense route); y = 0: minus_s = -C
    k.initialize()
    k.set_y(np.zeros(1))
    k.enable_timing(True)
    return k


def once(k, slot, call):
    for s in ("query", "prepare", "take"):
        k.kernel_clock(s, reset=True)
    call()
    k.sync()
    cnt, ms = k.kernel_clock(slot, reset=True)
    assert cnt == 1, (slot, cnt)
    return ms * 1e3


def stage_calls(k, step):
    def take():
        k.set_identity()
        k.prepare_step(None, 1.0, 1.0)
        k.take_step(step, 1.0)

    return {"query": lambda: k.weighted_slack_eigenvalues(None, 1.0), "prepare": lambda: k.prepare_step(None, 1.0, 1.0),
            "take": take}


def measure(n, modes, stages, rounds, warmup, slack=long_slack, slow=None):
    """slow: (mode, rounds) that gets that many rounds and no warm-up."""
    rng = np.random.default_rng(1)
    S = slack(n, rng)
    runs = {name: context(n, S, mode) for name, mode in modes.items()}
    calls = {name: stage_calls(k, 0.5) for name, k in runs.items()}
    times = {name: {s: [] for s in stages} for name in runs}
    for r in range(warmup + rounds):
        for name, k in runs.items():   # the runs alternate within a round
            if slow and name == slow[0]:
                if r >= slow[1]:
                    continue
                for s in stages:
                    times[name][s].append(once(k, s, calls[name][s]))
                continue
            for s in stages:
                us = once(k, s, calls[name][s])
                if r >= warmup:
                    times[name][s].append(us)
    out = {"n": n, "rounds": rounds}
    if slow:
        out[f"rounds_{slow[0]}"] = min(slow[1], warmup + rounds)
    for name, k in runs.items():
        for s in stages:
            out[f"{s}_{name}_us"] = round(float(np.median(times[name][s])), 1)
        k.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spectrum", type=int, nargs="*", help="orders for query and PrepareStep on both runs")
    ap.add_argument("--wide-only", type=int, nargs="*", help="orders for the chip-wide run alone")
    ap.add_argument("--take", type=int, nargs="*", help="orders for TakeStep")
    ap.add_argument("--short", type=int, nargs="*", help="orders for a chip-wide run that breaks at step 3")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slow-from", type=int, default=1500, help="orders from which the one-workgroup run gets --slow-rounds")
    ap.add_argument("--slow-rounds", type=int, default=1)
    a = ap.parse_args()
    if a.spectrum is None and a.wide_only is None and a.take is None and a.short is None:
        a.spectrum, a.wide_only, a.take, a.short = SPECTRUM_ORDERS, WIDE_ONLY_ORDERS, TAKE_ORDERS, (2550,)
    for n in a.spectrum or ():
        assert n <= MAX_ONE_WORKGROUP, "the one-workgroup run ends at order 2549: use --wide-only"
        slow = ("one", a.slow_rounds) if n >= a.slow_from else None
        print(json.dumps(measure(n, {"one": 0, "wide": 1}, ("query", "prepare"), a.rounds, a.warmup, slow=slow)), flush=True)
    for n in a.wide_only or ():
        print(json.dumps(measure(n, {"wide": 1}, ("query", "prepare"), a.rounds, a.warmup)), flush=True)
    for n in a.short or ():
        out = measure(n, {"wide": 1}, ("query",), a.rounds, a.warmup, slack=short_slack)
        per = 3 if n >= 2049 else 2  # (pass, [reduce from order 2049 on,] step) x (1 + n / 2); traces, start, finish
        out["launches"] = per * (n // 2 + 1) + 3
        out["us_per_launch"] = round(out["query_wide_us"] / out["launches"], 2)
        print(json.dumps(out), flush=True)
    for n in a.take or ():
        print(json.dumps(measure(n, {"wide": 1}, ("take",), a.rounds, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
