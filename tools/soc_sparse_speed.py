"""Kernel times of a second-order cone on the sparse route (kernels_soc_sparse.hip.h) against the dense routes.

  python tools/soc_sparse_speed.py --rows 8192 --unknowns 2048 --per-row 4       # |A x - b| <= t, both routes of this build
  python tools/soc_sparse_speed.py --rows 8192 --unknowns 2048 --per-row 4 --parent-lib /path/to/parent/libconex.so
  python tools/soc_sparse_speed.py --sweep                                       # the shapes behind the automatic rule

The cone is that of min t s.t. |A x - b| <= t over y = (x, t): dimension rows + 1, m = unknowns + 1 variables, row 0
holding the t column only, every other row --per-row entries (or a --fill fraction of all columns).

Times come from the library's kernel clocks (cxk_kernel_clock: hipEvent pairs around the launches of a stage): the
median over --rounds calls after --warmup.  Without --parent-lib both routes are built in one process (mode 1, and mode
0 with the streamed cones on: the LDS route where the cone fits it, the streamed route otherwise) and their rounds
alternate, so both see the same box in the same state.  With --parent-lib the dense route runs on that library (a build
from before the sparse route, on its own choice), each build in fresh processes, --pairs alternating pairs, the medians
of the pairs' medians reported.  Prints one JSON line per shape: microseconds per stage and route, the speed-ups, the
sparse assembly's share of its byte bound (16 m^2 bytes, H read and G written, at the data sheet's 8 TB/s),
len m / nnz and len m^2 (what the automatic rule compares with kSparseSocMinRatio and kSparseSocMinWork), the wall time
of initialize() and, for the sparse route, h_setup_us: the device time of the one-off H = A' J A, h and z in it.
--sweep takes shapes beyond LDS only: the LDS route's assembly carries no kernel clock.
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

HBM_PEAK = 8.0e12  # bytes/s, MI355X data sheet
STAGES = ("assembly", "query", "prepare", "take")
# (rows, unknowns, per_row or None, fill or None)
SWEEP = [
    (400, 60, 3, None),
    (400, 60, None, 0.25),
    (400, 60, None, 1.0),
    (1500, 200, 3, None),
    (2047, 63, 3, None),
    (2047, 63, None, 0.25),
    (2047, 63, None, 0.5),
    (3000, 64, 4, None),
    (8192, 2048, 4, None),
]  # (every shape is beyond LDS: the LDS route's assembly carries no kernel clock)


def cone_matrix(rows, unknowns, per_row, fill, rng):
    m = unknowns + 1
    M = np.zeros((rows + 1, m))
    M[0, unknowns] = -1.0
    if fill is not None:
        M[1:, :unknowns] = rng.uniform(-1, 1, (rows, unknowns)) * (rng.random((rows, unknowns)) < fill)
    else:
        cols = np.argsort(rng.random((rows, unknowns)), axis=1)[:, :per_row]  # distinct columns per row
        M[np.arange(1, rows + 1)[:, None], cols] = rng.uniform(-1, 1, (rows, per_row))
    return M


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


def context(a, route):
    from conex_amd import KktContext
    rng = np.random.default_rng(1)
    M = cone_matrix(a.rows, a.unknowns, a.per_row, a.fill, rng)
    length, m = M.shape
    k = KktContext(m, device=0)
    has_switch = hasattr(k.L, "cxk_set_sparse_soc")
    k.set_streamed_cones()
    if has_switch:
        k.set_sparse_soc(1 if route == "sparse" else 0)
    c = 0.2 * rng.uniform(-1, 1, length)
    c[0] = 1.0
    assert k.add_soc(M, c) == 0
    nnz = int(np.count_nonzero(M))
    del M
    t = time.perf_counter()
    k.initialize()
    k.sync()
    init_ms = (time.perf_counter() - t) * 1e3
    sparse = k.count_sparse_soc() if has_switch else 0
    assert sparse == (route == "sparse"), (route, sparse)
    ran = "sparse" if sparse else "streamed" if k.count_streamed_cones() else "lds"
    w = np.r_[1.0, rng.uniform(-1, 1, length - 1) * (0.5 / np.sqrt(length))]
    k.set_W(0, w)
    k.set_y(rng.uniform(-1, 1, k.N) * (0.25 / max(1, a.per_row or int(a.fill * a.unknowns))))
    k.enable_timing(True)
    setup_us = k.sparse_soc_setup_ms() * 1e3 if has_switch and hasattr(k.L, "cxk_sparse_soc_setup_ms") else 0.0
    return k, w, {"route": ran, "initialize_ms": round(init_ms, 1), "nnz": nnz, "setup_us": round(setup_us, 1)}


def stage_calls(k, w):
    def prepare():   # (PrepareStep leaves w^{1/2} in W: the same W every round)
        k.set_W(0, w)
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


def measure(a, routes):
    length, m = a.rows + 1, a.unknowns + 1
    out = {"rows": a.rows, "unknowns": a.unknowns, "per_row": a.per_row, "fill": a.fill, "rounds": a.rounds}
    built = {name: context(a, name) for name in routes}
    calls = {name: stage_calls(k, w) for name, (k, w, _) in built.items()}
    times = {name: {s: [] for s in STAGES} for name in built}
    for r in range(a.warmup + a.rounds):
        for name, (k, _, _) in built.items():   # the routes alternate within a round
            for s in STAGES:
                us = once(k, s, calls[name][s])
                if r >= a.warmup:
                    times[name][s].append(us)
    for name, (k, _, info) in built.items():
        out[f"{name}_route"], out[f"{name}_initialize_ms"], nnz = info["route"], info["initialize_ms"], info["nnz"]
        if name == "sparse":
            out["h_setup_us"] = info["setup_us"]  # (the one-off H = A' J A, h, z at initialize, device time)
        for s in STAGES:
            out[f"{s}_{name}_us"] = round(float(np.median(times[name][s])), 2)
        k.close()
    out["len_m_over_nnz"] = round(length * m / nnz, 2)
    out["len_m_m"] = length * m * m
    return finish(out)


def finish(out):
    m = out["unknowns"] + 1
    if "assembly_sparse_us" in out:
        out["assembly_share_of_byte_bound"] = round(16.0 * m * m / HBM_PEAK / (out["assembly_sparse_us"] * 1e-6), 4)
    if "assembly_sparse_us" in out and "assembly_dense_us" in out:
        for s in STAGES:
            out[f"speedup_{s}"] = round(out[f"{s}_dense_us"] / out[f"{s}_sparse_us"], 2)
        # take is measured behind prepare's W: an iteration costs assembly + query + prepare + take
        for name in ("sparse", "dense"):
            out[f"iteration_{name}_us"] = round(sum(out[f"{s}_{name}_us"] for s in STAGES), 2)
    return out


def child(a, route, parent):
    cmd = [sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--unknowns", str(a.unknowns), "--route", route,
           "--rounds", str(a.rounds), "--warmup", str(a.warmup)]
    cmd += ["--fill", str(a.fill)] if a.fill is not None else ["--per-row", str(a.per_row)]
    env = dict(os.environ)
    env.pop("CONEX_AMD_LIB", None)
    if parent:
        env["CONEX_AMD_LIB"] = a.parent_lib
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    if r.returncode != 0:  # nothing more is started after a failed process
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"{' '.join(cmd)} ended with {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def against_parent(a):
    runs = {"dense": [], "sparse": []}
    for _ in range(a.pairs):
        runs["dense"].append(child(a, "dense", True))
        runs["sparse"].append(child(a, "sparse", False))
    out = {k: runs["sparse"][0][k] for k in ("rows", "unknowns", "per_row", "fill", "rounds", "len_m_over_nnz", "len_m_m")}
    out["pairs"] = a.pairs
    out["h_setup_us"] = round(float(np.median([r["h_setup_us"] for r in runs["sparse"]])), 1)
    for name in ("dense", "sparse"):
        out[f"{name}_route"] = runs[name][0][f"{name}_route"]
        out[f"{name}_initialize_ms"] = round(float(np.median([r[f"{name}_initialize_ms"] for r in runs[name]])), 1)
        for s in STAGES:
            out[f"{s}_{name}_us"] = round(float(np.median([r[f"{s}_{name}_us"] for r in runs[name]])), 2)
    print(json.dumps(finish(out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--unknowns", type=int, default=2048)
    ap.add_argument("--per-row", type=int, default=4)
    ap.add_argument("--fill", type=float, default=None, help="fraction of nonzero entries instead of --per-row")
    ap.add_argument("--route", default="both", choices=("both", "sparse", "dense"))
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--child-timeout", type=float, default=300.0)
    a = ap.parse_args()
    if a.fill is not None:
        a.per_row = None
    if a.parent_lib:
        against_parent(a)
        return
    if os.environ.get("CONEX_AMD_LIB"):
        load_other_library()
    routes = ("sparse", "dense") if a.route == "both" else (a.route,)
    if a.sweep:
        for a.rows, a.unknowns, a.per_row, a.fill in SWEEP:
            print(json.dumps(measure(a, routes)), flush=True)
    else:
        print(json.dumps(measure(a, routes)), flush=True)


if __name__ == "__main__":
    main()
