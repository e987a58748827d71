"""Kernel times of the streamed second-order cone path (kernels_soc_stream.hip.h) at one shape.

  python tools/soc_stream_speed.py --cones 1 --n 100000 --m 64     # one big cone
  python tools/soc_stream_speed.py --cones 64 --n 2000 --m 32      # a batch

Times come from the library's kernel clocks (cxk_kernel_clock: hipEvent pairs around the launches of a
stage).  The three stages of the Schur assembly are separated by difference: the assembly is timed with
CXK_SOC_STREAM_STAGES=1 (vectors only), =2 (vectors + apply) and unset (all four launches), each in a fresh
context.  Prints one JSON line: microseconds per stage (median over the rounds, after warm-up), the Gram
stage's fraction of the fp64 MFMA bound (2 len m^2 flops per cone) and the apply stage's fraction of the HBM
bound (len m 8 bytes read and as many written per cone).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MFMA_F64_PEAK = 78.6e12   # flop/s, MI355X dense fp64 matrix (the bound bench.py's roofline uses is measured; this is the data sheet's)
HBM_PEAK = 8.0e12         # bytes/s, MI355X data sheet


def context(a, stages):
    from conex_amd import KktContext, synthetic as syn
    if stages:
        os.environ["CXK_SOC_STREAM_STAGES"] = str(stages)
    else:
        os.environ.pop("CXK_SOC_STREAM_STAGES", None)
    rng = np.random.default_rng(1)
    cliques, num_vars = syn.chain_cliques(a.cones, a.m, 1 if a.m > 1 else 0)
    k = KktContext(num_vars, device=0)
    k.set_streamed_cones()
    for cl in cliques:
        A = rng.uniform(-1, 1, (a.n + 1, a.m))
        c = 0.2 * rng.uniform(-1, 1, a.n + 1)
        c[0] = 1.0
        assert k.add_soc(A, c, cl) >= 0
    k.initialize()
    assert k.count_streamed_cones() == a.cones, "this shape fits LDS: it does not take the streamed kernels"
    for i in range(a.cones):
        w = rng.uniform(-1, 1, a.n + 1)
        w[0] = 2.0 * np.linalg.norm(w[1:])
        k.set_W(i, w / w[0])
    y = rng.uniform(-1, 1, k.N)
    y *= 0.25 / (a.m * 1.0)
    k.set_y(y)
    return k


def clocked(k, slot, rounds, warmup, call):
    """Median of per-call samples of one clock slot, in microseconds."""
    k.enable_timing(True)
    out = []
    for r in range(warmup + rounds):
        call()
        k.sync()
        n, ms = k.kernel_clock(slot, reset=True)
        assert n == 1, (slot, n)
        if r >= warmup:
            out.append(ms * 1e3)
    k.enable_timing(False)
    return float(np.median(out)), float(np.min(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cones", type=int, default=1)
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    out = {"cones": a.cones, "n": a.n, "m": a.m, "rounds": a.rounds}
    asm = {}
    for stages in (1, 2, 0):
        k = context(a, stages)
        asm[stages] = clocked(k, "assembly", a.rounds, a.warmup, k.assemble)[0]
        if stages == 0:
            w = [k.get_W(i) for i in range(a.cones)]
            out["query_us"] = clocked(k, "query", a.rounds, a.warmup, lambda: k.weighted_slack_eigenvalues(None, 1.0))[0]

            def prepare():   # (PrepareStep leaves w^{1/2} in W: the same W every round)
                for i in range(a.cones):
                    k.set_W(i, w[i])
                k.prepare_step(None, 1.0, 1.0)
            out["prepare_us"] = clocked(k, "prepare", a.rounds, a.warmup, prepare)[0]

            def take():
                prepare()
                k.take_step(0.5, 1.0)
            out["take_us"] = clocked(k, "take", a.rounds, a.warmup, take)[0]
        k.close()
    length = a.n + 1
    out["vectors_us"] = asm[1]
    out["apply_us"] = asm[2] - asm[1]
    out["gram_us"] = asm[0] - asm[2]
    out["assembly_us"] = asm[0]
    out["gram_fraction_of_mfma_peak"] = 2.0 * length * a.m * a.m * a.cones / (out["gram_us"] * 1e-6) / MFMA_F64_PEAK
    out["apply_fraction_of_hbm_peak"] = 2.0 * 8.0 * length * a.m * a.cones / (out["apply_us"] * 1e-6) / HBM_PEAK
    print(json.dumps(out))


if __name__ == "__main__":
    main()
