"""Host wall times of the three stages a linear-inequality block costs per iteration, at one shape, on one route.

  python tools/linear_tiled_speed.py --blocks 1 --rows 1100 --m 960 --mode 1     # the tiled route
  python tools/linear_tiled_speed.py --blocks 1000 --rows 20 --m 10 --mode 0     # the LDS route

Times are host wall clock around assemble(); sync(), prepare_step and weighted_slack_eigenvalues (both wait for
their results): the median of --rounds calls after --warmup.  The switch is used only if the loaded library has
it, so the same script times a build from before the tiled route (CONEX_AMD_LIB names another library file);
"route" in the output says what ran.  Prints one JSON line; assembly_fraction_of_mfma_peak is the Gram product's
2 rows m^2 flops per block over the WHOLE assembly's time (scalars, apply, Gram and mirror together: the stages are
not timed apart, so the Gram stage alone runs at no less than this fraction) next to the fp64 MFMA peak.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MFMA_F64_PEAK = 78.6e12   # flop/s, MI355X dense fp64 matrix (data sheet)


def median_us(call, rounds, warmup):
    out = []
    for r in range(warmup + rounds):
        t = time.perf_counter()
        call()
        if r >= warmup:
            out.append((time.perf_counter() - t) * 1e6)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1)
    ap.add_argument("--rows", type=int, default=1100)
    ap.add_argument("--m", type=int, default=960)
    ap.add_argument("--mode", type=int, default=1, choices=(-1, 0, 1))
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if os.environ.get("CONEX_AMD_LIB"):
        import ctypes
        import conex_amd.kkt as kkt
        path = os.environ["CONEX_AMD_LIB"]
        has = hasattr(ctypes.CDLL(path), "cxk_set_tiled_linear")
        if not has:  # a library from before the switch: its table must not ask for the two calls
            for name in ("cxk_set_tiled_linear", "cxk_count_tiled_linear"):
                kkt._SIGNATURES.pop(name, None)
        kkt.LIB_PATH = path
    from conex_amd import KktContext, synthetic as syn
    rng = np.random.default_rng(1)
    cliques, num_vars = syn.chain_cliques(a.blocks, a.m, 1 if a.m > 1 else 0)
    k = KktContext(num_vars, device=0)
    has_switch = hasattr(k.L, "cxk_set_tiled_linear")
    if has_switch:
        k.set_tiled_linear(a.mode)
    for cl in cliques:
        assert k.add_linear(rng.uniform(-1, 1, (a.rows, a.m)), np.abs(rng.uniform(-1, 1, a.rows)) + 0.1, cl) >= 0
    k.initialize()
    tiled = k.count_tiled_linear() if has_switch else 0
    for i in range(a.blocks):
        k.set_W(i, rng.uniform(0.5, 1.5, a.rows))
    y = rng.uniform(-1, 1, k.N) * (0.25 / a.m)
    k.set_y(y)

    def assemble():
        k.assemble()
        k.sync()

    out = {"blocks": a.blocks, "rows": a.rows, "m": a.m, "rounds": a.rounds,
           "route": "tiled" if tiled == a.blocks else "lds" if tiled == 0 else "mixed", "has_switch": has_switch}
    out["assemble_us"] = median_us(assemble, a.rounds, a.warmup)
    out["prepare_us"] = median_us(lambda: k.prepare_step(None, 1.0, 1.0), a.rounds, a.warmup)
    out["query_us"] = median_us(lambda: k.weighted_slack_eigenvalues(None, 1.0), a.rounds, a.warmup)
    out["assembly_fraction_of_mfma_peak"] = 2.0 * a.rows * a.m * a.m * a.blocks / (out["assemble_us"] * 1e-6) / MFMA_F64_PEAK
    k.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
