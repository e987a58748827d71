"""One block solve of 32 columns against 32 single solves on the default lmi_problem() (BASELINE config 4).

  python tools/solve_block_speed.py --mode block                 # cxk_solve_block_device on a resident block + cxk_sync
  python tools/solve_block_speed.py --mode single [--lib PATH]   # 32 x cxk_solve_rhs + one cxk_sync

The yardstick (--mode single) is meant to be run with the PARENT commit's library (--lib), alternating with
--mode block in separate processes on the same device.  Host wall time around enqueue + sync, after warm-up;
prints one JSON line with the median and the minimum over the rounds.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("block", "single"), required=True)
    ap.add_argument("--lib", default=None, help="another libconex.so (the parent commit's) for --mode single")
    ap.add_argument("--nrhs", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if a.mode == "block":
        import torch
        torch.cuda.init()   # torch's GPU state before the library's (the order bench.py uses)
    from conex_amd import kkt
    if a.lib:
        kkt.LIB_PATH = os.path.abspath(a.lib)
        if a.mode == "single":   # the parent's library has no block solve to declare
            for name in [n for n in kkt._SIGNATURES if n.startswith("cxk_solve_block")]:
                del kkt._SIGNATURES[name]
    from conex_amd import KktContext, synthetic as syn
    prob = syn.lmi_problem()
    W = syn.scaling_points(1000, 20)
    k = syn.build(KktContext, prob, "lmi", device=0)
    for i in range(k.K):
        k.set_W(i, W[i])
    k.set_cost(prob["b"])
    k.assemble()
    assert k.factor() == 1
    out = {"mode": a.mode, "nrhs": a.nrhs, "N": k.N, "lib": kkt.LIB_PATH}
    if a.mode == "block":
        out["chunk_width"] = int(k.L.cxk_solve_block_chunk_width())
        B = np.random.default_rng(0).uniform(-1, 1, (k.N, a.nrhs))
        t0 = torch.from_numpy(B).to("cuda:0").T.contiguous().T
        t = t0.clone()
        torch.cuda.synchronize()
        ptr = C.c_void_p(t.data_ptr())

        def once():
            k._check(k.L.cxk_solve_block_device(k.h, ptr, k.N, a.nrhs), "cxk_solve_block_device")
            k.sync()
    else:
        def once():
            for j in range(a.nrhs):
                k._check(k.L.cxk_solve_rhs(k.h, 1.0 + 0.01 * j, 0.5, -2.0), "cxk_solve_rhs")
            k.sync()
    times = []
    for r in range(a.warmup + a.rounds):
        if a.mode == "block":
            t.copy_(t0)          # (the solve is in place: a fresh right-hand side every round)
            torch.cuda.synchronize()
        s = time.perf_counter()
        once()
        e = time.perf_counter()
        if r >= a.warmup:
            times.append((e - s) * 1e6)
    out["median_us"] = float(np.median(times))
    out["min_us"] = float(np.min(times))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
