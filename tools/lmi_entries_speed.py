"""Assembly time of a sparse matrix inequality whose affine term is evaluated from its nonzeros (cxk_set_sparse_affine,
kernels_lmi_sparse.hip.h: lmi_affine_wc / _x / _scalars) against the two GEMMs it replaces.

  python tools/lmi_entries_speed.py --family maxcut --n 2000        # synthetic.maxcut_entries, n = m
  python tools/lmi_entries_speed.py --family band --n 1024 --band 8 # C with 8 sub-diagonals, A_i = -e_i e_i^T
  python tools/lmi_entries_speed.py --family fill --n 256 --fill 0.25   # a fraction of C's entries: the threshold sweep
  python tools/lmi_entries_speed.py --sweep                         # the fill family over the ratios behind the rule
  python tools/lmi_entries_speed.py --family maxcut --n 500 --parent-lib /path/to/parent/libconex.so

Every constraint is built through KktContext.add_lmi_coo, so nothing of size m n^2 exists on the host; the line
reports the process's peak resident set (ru_maxrss) after both contexts are built.  Times come from the assembly kernel
clock (cxk_kernel_clock(CXK_CLOCK_ASSEMBLY): a hipEvent pair around the launches of the group): --warmup rounds, then
the median of --rounds, the two modes alternating within a round, and that --runs times: the medians of the runs'
medians are reported, with the ratio 4 n^2 / (nnz C + positions) that LmiSparseAffinePays compares with its constant.
The clock covers the group's launches together, so the two shares printed are of the whole assembly (the three new
launches and lmi_schur_sparse) against the two new kernels' bounds: an underestimate of each kernel's own share, which
a run of this tool with --mode 1 under rocprofv3 --kernel-trace --stats gives from the kernels' own times.
 - HBM bound: lmi_affine_wc reads W once and writes U (16 n^2 bytes); lmi_affine_x reads a column of U and of W per
   position at worst (16 n |P| bytes; neighbouring positions share U's column, and both matrices fit the 256 MB of
   MALL up to n = 4000, so this is an upper bound on HBM traffic); data sheet 8 TB/s.
 - issue bound: n (nnz C + |P|) fused multiply-adds, one per lane and cycle on 256 CUs x 4 SIMDs x 16 lanes at 2.4 GHz.
--parent-lib: the same data given densely to cxk_add_lmi on that library (a build from before this entry point), in a
fresh process, on its own choice of route; only for orders whose m n^2 doubles fit the host.
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

HBM_PEAK = 8.0e12          # bytes/s, MI355X data sheet
FMA_PEAK = 256 * 4 * 16 * 2.4e9  # fp64 fused multiply-adds/s on the vector pipe
SWEEP = [(256, 1.0), (256, 0.5), (256, 0.25), (256, 0.1), (256, 0.03), (512, 1.0), (512, 0.25), (1024, 0.5), (1024, 0.1)]


def entries(a):
    """ptr, row, col, val of the family: A_i = -e_i e_i^T (i < n), then the lower triangle of C."""
    from conex_amd import synthetic as syn
    n = a.n
    if a.family == "maxcut":
        e = syn.maxcut_entries(n)
        return e["ptr"], e["row"], e["col"], e["val"]
    rng = np.random.default_rng(5 + n)
    if a.family == "band":
        r = np.concatenate([np.arange(d, n) for d in range(1, a.band + 1)])
        c = np.concatenate([np.arange(0, n - d) for d in range(1, a.band + 1)])
    else:
        r, c = np.tril_indices(n, -1)
        keep = rng.random(len(r)) < a.fill
        r, c = r[keep], c[keep]
    v = rng.uniform(0.05, 0.25, len(r)) / max(1, len(r) / n)
    row = np.r_[np.arange(n), np.arange(n), r].astype(np.int32)
    col = np.r_[np.arange(n), np.arange(n), c].astype(np.int32)
    val = np.r_[-np.ones(n), np.ones(n), v]
    ptr = np.r_[np.arange(n + 1), len(row)].astype(np.int32)
    return ptr, row, col, val


def scaling_point(n):
    rng = np.random.default_rng(n)
    S = rng.standard_normal((n, n))
    return np.eye(n) + 0.3 * 0.5 * (S + S.T) / np.sqrt(n)


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


def context(a, mode, lists, W):
    from conex_amd import KktContext
    ptr, row, col, val = lists
    k = KktContext(a.n, device=0)
    t = time.perf_counter()
    if mode == "dense-entry":  # (the parent's only way in)
        A = np.zeros((a.n, a.n, a.n))
        A[np.arange(a.n), np.arange(a.n), np.arange(a.n)] = -1.0
        Cm = np.zeros((a.n, a.n))
        s = slice(ptr[a.n], ptr[a.n + 1])
        Cm[row[s], col[s]] = val[s]
        Cm[col[s], row[s]] = val[s]
        assert k.add_lmi(A, Cm) == 0
        del A
    else:
        k.set_sparse_affine(mode)
        assert k.add_lmi_coo(a.n, ptr, row, col, val) == 0
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
    lists = entries(a)
    n = a.n
    nnz_c = int(2 * (lists[0][n + 1] - lists[0][n]) - np.count_nonzero(lists[1][lists[0][n]:] == lists[2][lists[0][n]:]))
    W = scaling_point(n)
    out = {"family": a.family, "n": n, "nnz_c": nnz_c, "rounds": a.rounds, "runs": a.runs}
    if a.family == "band":
        out["band"] = a.band
    if a.family == "fill":
        out["fill"] = a.fill
    modes = ("dense-entry",) if a.mode == "dense-entry" else (0, 1) if a.mode == "both" else (int(a.mode),)
    built = {}
    for mode in modes:
        built[mode], out[f"initialize_ms_mode_{mode}"] = context(a, mode, lists, W)
        out[f"initialize_ms_mode_{mode}"] = round(out[f"initialize_ms_mode_{mode}"], 1)
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
    for mode, k in built.items():
        out[f"assembly_us_mode_{mode}"] = round(float(np.median(medians[mode])), 2)
        out[f"kernel_mode_{mode}"] = k.lmi_kernels(0)["schur"]
        k.close()
    # positions: the diagonal (every A_i) and C's pattern
    npos = nnz_c + n - int(np.count_nonzero(lists[1][lists[0][n]:] == lists[2][lists[0][n]:]))
    out["positions"] = npos
    out["ratio_4nn_over_nnz_plus_positions"] = round(4.0 * n * n / (nnz_c + npos), 2)
    if 0 in built and 1 in built:
        out["speedup"] = round(out["assembly_us_mode_0"] / out["assembly_us_mode_1"], 2)
    if 1 in built:
        t = out["assembly_us_mode_1"] * 1e-6
        out["share_of_hbm_bound"] = round((16.0 * n * n + 16.0 * n * npos) / HBM_PEAK / t, 4)
        out["share_of_issue_bound"] = round(n * float(nnz_c + npos) / FMA_PEAK / t, 4)
    return out


def child(a, env_lib):
    cmd = [sys.executable, os.path.abspath(__file__), "--family", a.family, "--n", str(a.n), "--band", str(a.band), "--fill",
           str(a.fill), "--rounds", str(a.rounds), "--warmup", str(a.warmup), "--runs", str(a.runs), "--mode", "dense-entry"]
    env = dict(os.environ)
    env["CONEX_AMD_LIB"] = env_lib
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    if r.returncode != 0:  # nothing more is started after a failed process
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"{' '.join(cmd)} ended with {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", default="maxcut", choices=("maxcut", "band", "fill"))
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--band", type=int, default=8)
    ap.add_argument("--fill", type=float, default=0.25)
    ap.add_argument("--mode", default="both", choices=("both", "0", "1", "dense-entry"))
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child-timeout", type=float, default=300.0)
    a = ap.parse_args()
    if os.environ.get("CONEX_AMD_LIB"):
        load_other_library()
    if a.sweep:
        a.family = "fill"
        for a.n, a.fill in SWEEP:
            print(json.dumps(measure(a)), flush=True)
        return
    out = measure(a)
    if a.parent_lib:
        p = child(a, a.parent_lib)
        out["parent_dense_entry_us"] = p["assembly_us_mode_dense-entry"]
        out["parent_kernel"] = p["kernel_mode_dense-entry"]
        out["parent_peak_rss_mb"] = p["peak_rss_mb"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
