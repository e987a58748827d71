"""Host wall times of the three stages a linear-inequality block costs per iteration, at one shape and pattern, on
the sparse route or on whatever another build chooses by itself.

  python tools/linear_sparse_speed.py --pattern bounds --m 4096 --mode 1          # [I; -I], the sparse route
  CONEX_AMD_LIB=/path/to/parent/libconex.so python tools/linear_sparse_speed.py --pattern bounds --m 4096
  python tools/linear_sparse_speed.py --sweep --parent-lib /path/to/parent/libconex.so

Times are host wall clock around assemble(); sync(), prepare_step and weighted_slack_eigenvalues (both wait for
their results): the median of --rounds calls after --warmup, the protocol of tools/linear_tiled_speed.py.  The
sparse switch is used only if the loaded library has it, so the same script times the build from before the sparse
route (CONEX_AMD_LIB names its library file) on its own automatic choice between the LDS and the tiled route;
"route" in the output says what ran.  Prints one JSON line.

--sweep runs the shapes of DESIGN.md 4.4.3, each as three alternating pairs of fresh processes (the parent build,
then this build in mode 1), and prints per shape the medians of the three, the stage-wise speed-ups and
rows m^2 / sum_r nnz_r^2, the quantity the automatic rule compares with kSparseLinearMinRatio.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (pattern, blocks, rows, m)
SWEEP = [
    ("bounds", 1, 512, 256),
    ("bounds", 1, 2048, 1024),
    ("bounds", 1, 8192, 4096),
    ("per-row3", 1, 20000, 200),
    ("per-row3", 1000, 20, 10),
    ("half", 1, 2000, 64),
    ("dense", 1, 400, 300),
    ("dense-col", 1, 100000, 50),
]
STAGES = ("assemble_us", "prepare_us", "query_us")


def make_block(pattern, rows, m, rng):
    if pattern == "bounds":
        assert rows == 2 * m
        return np.vstack([np.eye(m), -np.eye(m)])
    if pattern == "dense":
        return rng.uniform(-1, 1, (rows, m))
    if pattern == "half":
        return rng.uniform(-1, 1, (rows, m)) * (rng.random((rows, m)) < 0.5)
    per_row = 3 if pattern == "per-row3" else 2
    first = 1 if pattern == "dense-col" else 0
    A = np.zeros((rows, m))
    cols = np.argsort(rng.random((rows, m - first)), axis=1)[:, :per_row] + first  # distinct columns per row
    A[np.arange(rows)[:, None], cols] = rng.uniform(-1, 1, (rows, per_row))
    if pattern == "dense-col":
        A[:, 0] = rng.uniform(-1, 1, rows)
    return A


def median_us(call, rounds, warmup):
    out = []
    for r in range(warmup + rounds):
        t = time.perf_counter()
        call()
        if r >= warmup:
            out.append((time.perf_counter() - t) * 1e6)
    return float(np.median(out))


def measure(a):
    if os.environ.get("CONEX_AMD_LIB"):
        import ctypes
        import conex_amd.kkt as kkt
        path = os.environ["CONEX_AMD_LIB"]
        lib = ctypes.CDLL(path)
        for name in list(kkt._SIGNATURES):  # a library from before a call: its table must not ask for it
            if not hasattr(lib, name):
                kkt._SIGNATURES.pop(name)
        kkt.LIB_PATH = path
    from conex_amd import KktContext, synthetic as syn
    rng = np.random.default_rng(1)
    cliques, num_vars = syn.chain_cliques(a.blocks, a.m, 1 if a.m > 1 else 0)
    k = KktContext(num_vars, device=0)
    has_switch = hasattr(k.L, "cxk_set_sparse_linear")
    if has_switch:
        k.set_sparse_linear(a.mode)
    ratio = []
    for cl in cliques:
        A = make_block(a.pattern, a.rows, a.m, rng)
        ratio.append(float(a.rows) * a.m * a.m / max(1.0, float(np.sum(np.count_nonzero(A, axis=1).astype(np.float64) ** 2))))
        assert k.add_linear(A, np.abs(rng.uniform(-1, 1, a.rows)) + 0.1, cl) >= 0
        del A
    k.initialize()
    sparse = k.count_sparse_linear() if has_switch else 0
    tiled = k.count_tiled_linear()
    for i in range(a.blocks):
        k.set_W(i, rng.uniform(0.5, 1.5, a.rows))
    k.set_y(rng.uniform(-1, 1, k.N) * (0.25 / a.m))

    def assemble():
        k.assemble()
        k.sync()

    route = "sparse" if sparse == a.blocks else "tiled" if tiled == a.blocks else "lds" if sparse + tiled == 0 else "mixed"
    out = {"pattern": a.pattern, "blocks": a.blocks, "rows": a.rows, "m": a.m, "rounds": a.rounds, "route": route,
           "has_switch": has_switch, "dense_over_sparse_work": min(ratio)}
    out["assemble_us"] = median_us(assemble, a.rounds, a.warmup)
    out["prepare_us"] = median_us(lambda: k.prepare_step(None, 1.0, 1.0), a.rounds, a.warmup)
    out["query_us"] = median_us(lambda: k.weighted_slack_eigenvalues(None, 1.0), a.rounds, a.warmup)
    k.close()
    print(json.dumps(out), flush=True)


def child(shape, a, parent):
    pattern, blocks, rows, m = shape
    cmd = [sys.executable, os.path.abspath(__file__), "--pattern", pattern, "--blocks", str(blocks), "--rows", str(rows),
           "--m", str(m), "--mode", "1", "--rounds", str(a.rounds), "--warmup", str(a.warmup)]
    env = dict(os.environ)
    env.pop("CONEX_AMD_LIB", None)
    if parent:
        env["CONEX_AMD_LIB"] = a.parent_lib
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    if r.returncode != 0:  # nothing more is started after a failed process
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"{' '.join(cmd)} ended with {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def sweep(a):
    for shape in SWEEP:
        runs = {True: [], False: []}
        for _ in range(a.pairs):
            for parent in (True, False):
                runs[parent].append(child(shape, a, parent))
        row = {"pattern": shape[0], "blocks": shape[1], "rows": shape[2], "m": shape[3],
               "dense_over_sparse_work": runs[False][0]["dense_over_sparse_work"],
               "parent_route": runs[True][0]["route"], "route": runs[False][0]["route"]}
        for s in STAGES:
            old = float(np.median([r[s] for r in runs[True]]))
            new = float(np.median([r[s] for r in runs[False]]))
            row["parent_" + s], row[s], row["speedup_" + s[:-3]] = round(old, 1), round(new, 1), round(old / new, 2)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pattern", default="bounds", choices=("bounds", "per-row3", "half", "dense", "dense-col"))
    ap.add_argument("--blocks", type=int, default=1)
    ap.add_argument("--rows", type=int, default=0, help="default: 2 m")
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--mode", type=int, default=1, choices=(-1, 0, 1))
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--child-timeout", type=float, default=120.0)
    a = ap.parse_args()
    if not a.rows:
        a.rows = 2 * a.m
    if a.sweep:
        if not a.parent_lib:
            raise SystemExit("--sweep needs --parent-lib")
        sweep(a)
    else:
        measure(a)


if __name__ == "__main__":
    main()
