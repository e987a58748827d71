"""Assembly time of a sparse Hermitian matrix inequality given by its entries (cxk_add_hermitian_coo) with the folded
sums of kernels_lmi_sparse.hip.h (cxk_set_sparse_fold) against the unfolded ones.

  python tools/lmi_hermitian_entries_speed.py --n 2000 --d 2            # the line family, m = n
  python tools/lmi_hermitian_entries_speed.py --n 500 --d 4
  python tools/lmi_hermitian_entries_speed.py --n 200 --d 2 --parent-lib /path/to/parent/libconex.so

The data is synthetic.hermitian_entries (per_matrix = 0: every A_i one bus and one line, C = I; --per-matrix k: k random
entries).  Every constraint is built through KktContext.add_hermitian_coo, so nothing of size m (d n)^2 exists on the
host; the line reports the process's peak resident set (ru_maxrss) after both contexts are built.  Times come from the
assembly kernel clock (cxk_kernel_clock(CXK_CLOCK_ASSEMBLY): a hipEvent pair around the launches of the group):
--warmup rounds, then the median of --rounds, folded and unfolded alternating within a round, and that --runs times: the
medians of the runs' medians are reported with the spread of the runs' medians (max - min), and the number of terms of
the pair sums in either form (top(longer) x full(shorter) against full x full).  The clock covers the group's launches
together: with C = I (d n nonzeros, more than 64) that is the two GEMMs of W C W, the slices of the two scalars and
lmi_schur_sparse, of which only the last changes; --affine 1 (cxk_set_sparse_affine) takes the GEMMs away.
--parent-lib: the same data given as dense planes to cxk_add_hermitian under CXK_SPARSE_LMI=1 on that library (a build
from before this entry point), in a fresh process; only for orders whose m (d n)^2 doubles fit the host.
"""
import argparse
import json
import os
import resource
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_other_library():
    """CONEX_AMD_LIB names another build's library file: its table must not ask for calls it does not have."""
    import ctypes
    import conex_amd.kkt as kkt
    path = os.environ["CONEX_AMD_LIB"]
    lib = ctypes.CDLL(path)
    for name in list(kkt._SIGNATURES):
        if not hasattr(lib, name):
            kkt._SIGNATURES.pop(name)
    kkt.LIB_PATH = path


def scaling_point(n, d):
    """Hermitian positive definite planes: I + a small Hermitian matrix."""
    rng = np.random.default_rng(n + d)
    W = np.zeros((d, n, n))
    S = rng.standard_normal((d, n, n)) * (0.15 / np.sqrt(d * n))
    W[0] = np.eye(n) + S[0] + S[0].T
    for p in range(1, d):
        W[p] = S[p] - S[p].T
    return W


def real_counts(e):
    """Per list: the nonzeros of the real representation (d^2 per off-diagonal plane and mirror, d per diagonal entry)."""
    d, out = e["d"], []
    for i in range(e["m"] + 1):
        s = slice(e["ptr"][i], e["ptr"][i + 1])
        off = e["row"][s] != e["col"][s]
        out.append(int(d * np.count_nonzero(e["val"][s][~off]) + 2 * d * np.count_nonzero(e["val"][s][off])))
    return out


def pair_terms(counts, d, cdense):
    c = np.array(counts[:-1] if cdense else counts, dtype=np.float64)
    hi, lo = np.maximum.outer(c, c), np.minimum.outer(c, c)
    full = float(np.sum(np.tril(hi * lo)))
    return full, full / d


def context(a, mode, e, W):
    from conex_amd import KktContext
    k = KktContext(a.m, device=0)
    if a.affine is not None:
        k.set_sparse_affine(a.affine)
    t = time.perf_counter()
    if mode == "planes":  # (the parent's only way in)
        from conex_amd import synthetic as syn
        A, Cm = syn.hermitian_planes_of_entries(a.n, a.d, a.m, e["ptr"], e["row"], e["col"], e["val"])
        assert k.add_hermitian(A, Cm) == 0
        del A
    else:
        k.set_sparse_fold(mode)
        assert k.add_hermitian_coo(a.n, a.d, e["ptr"], e["row"], e["col"], e["val"]) == 0
    k.initialize()
    k.sync()
    init_ms = (time.perf_counter() - t) * 1e3
    k.set_W(0, W)
    k.enable_timing(True)
    return k, init_ms


def once(k):
    k.kernel_clock("assembly", reset=True)
    k.assemble()
    k.sync()
    n, ms = k.kernel_clock("assembly", reset=True)
    assert n == 1, n
    return ms * 1e3


def measure(a):
    from conex_amd import synthetic as syn
    e = syn.hermitian_entries(a.n, a.d, a.m, per_matrix=a.per_matrix, planes_up_to=0)
    W = scaling_point(a.n, a.d)
    counts = real_counts(e)
    cdense = counts[-1] > 64
    full, folded = pair_terms(counts, a.d, cdense)
    out = {"n": a.n, "d": a.d, "m": a.m, "per_matrix": a.per_matrix, "real_nonzeros": int(sum(counts)), "rounds": a.rounds,
           "runs": a.runs, "sparse_affine": a.affine, "pair_terms_unfolded": full, "pair_terms_folded": folded}
    modes = ("planes",) if a.mode == "planes" else (0, 1) if a.mode == "both" else (int(a.mode),)
    built = {}
    for mode in modes:
        built[mode], ms = context(a, mode, e, W)
        out[f"initialize_ms_{mode}"] = round(ms, 1)
    out["peak_rss_mb"] = round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0, 1)
    medians = {mode: [] for mode in modes}
    for _ in range(a.runs):
        times = {mode: [] for mode in modes}
        for r in range(a.warmup + a.rounds):
            for mode in modes:  # the modes alternate within a round
                us = once(built[mode])
                if r >= a.warmup:
                    times[mode].append(us)
        for mode in modes:
            medians[mode].append(float(np.median(times[mode])))
    name = {0: "unfolded", 1: "folded", "planes": "planes"}
    for mode, k in built.items():
        out[f"assembly_us_{name[mode]}"] = round(float(np.median(medians[mode])), 2)
        out[f"spread_us_{name[mode]}"] = round(float(np.max(medians[mode]) - np.min(medians[mode])), 2)
        out[f"kernel_{name[mode]}"] = k.lmi_kernels(0)["schur"]
        k.close()
    if 0 in built and 1 in built:
        out["speedup"] = round(out["assembly_us_unfolded"] / out["assembly_us_folded"], 3)
    return out


def child(a, env_lib):
    cmd = [sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--d", str(a.d), "--m", str(a.m), "--per-matrix",
           str(a.per_matrix), "--rounds", str(a.rounds), "--warmup", str(a.warmup), "--runs", str(a.runs), "--mode", "planes"]
    if a.affine is not None:
        cmd += ["--affine", str(a.affine)]
    env = dict(os.environ)
    env["CONEX_AMD_LIB"] = env_lib
    env["CXK_SPARSE_LMI"] = "1"
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    if r.returncode != 0:  # nothing more is started after a failed process
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"{' '.join(cmd)} ended with {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--d", type=int, default=2, choices=(2, 4))
    ap.add_argument("--m", type=int, default=0, help="variables (default: n)")
    ap.add_argument("--per-matrix", type=int, default=0, help="0: the line family; k: k random entries a matrix")
    ap.add_argument("--mode", default="both", choices=("both", "0", "1", "planes"))
    ap.add_argument("--affine", type=int, default=None, choices=(-1, 0, 1),
                    help="cxk_set_sparse_affine (default: no call, the GEMMs behind W C W for these entry points)")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child-timeout", type=float, default=300.0)
    a = ap.parse_args()
    a.m = a.m or a.n
    if os.environ.get("CONEX_AMD_LIB"):
        load_other_library()
    out = measure(a)
    if a.parent_lib:
        p = child(a, a.parent_lib)
        out["parent_planes_us"] = p["assembly_us_planes"]
        out["parent_spread_us"] = p["spread_us_planes"]
        out["parent_kernel"] = p["kernel_planes"]
        out["parent_peak_rss_mb"] = p["peak_rss_mb"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
