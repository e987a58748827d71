"""Kernel times of a low-rank LMI given by factors (kernels_lmi_factored.hip.h) against its expansion on the dense route.

  python tools/lmi_factored_speed.py --n 200 --m 200                # rank one, both forms in one process
  python tools/lmi_factored_speed.py --n 200 --m 200 --dense        # the expanded form alone (runs on any build)
  python tools/lmi_factored_speed.py --n 200 --m 200 --parent-lib /path/to/parent/libconex.so
  python tools/lmi_factored_speed.py --sweep                        # n in {64, 200, 500}, m in {n/4, n, 4n}
  python tools/lmi_factored_speed.py --n 1000 --m 4000 --factored   # a shape the dense form cannot hold
  python tools/lmi_factored_speed.py --herm 2 --n 200 --m 200       # complex Hermitian: add_hermitian_factored against add_hermitian

One constraint of order n over m variables, A_i = f_i f_i' with dense Gaussian f_i (--rank r: r columns each), C = I,
W at the well-conditioned point of the LMI tests.  Times come from the library's kernel clocks (cxk_kernel_clock:
hipEvent pairs around the launches of a stage): the median over --rounds calls after --warmup.  Without --parent-lib
the forms named are built in one process and their rounds alternate.  With --parent-lib the expanded form runs on that
library (a build from before the factored route), each form in fresh processes, --pairs alternating pairs; every pair's
medians are printed, then the medians over the pairs.  Prints one JSON line per shape: microseconds per stage and form,
the speed-ups, the device bytes held for A and for F, and the route's own flop count (cxk_assembly_work).  A shape
whose expanded form exceeds --dense-limit-gb (8) is measured in the factored form only, and says so.
--herm d (2 or 4; 1 for the Hermitian rules over R): the f_i are hyper-complex, A_i = f_i f_i^*, the factored form is
add_hermitian_factored and the expanded one add_hermitian on the d planes of every A_i; both hold their data in the real
representation of order d n on the device (m (d n)^2 doubles against d n x d R).
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("assembly", "query", "prepare", "take")
SWEEP = [(n, m) for n in (64, 200, 500) for m in (n // 4, n, 4 * n)]


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


def dense_bytes(n, m, d=1):
    return 8.0 * m * (d * n) * (d * n)


def hermitian_context(a, form):
    from conex_amd import KktContext
    from conex_amd import synthetic as syn
    rng = np.random.default_rng(1)
    n, m, d, R = a.n, a.m, a.herm, a.m * a.rank
    F = rng.standard_normal((d, n, R)) / np.sqrt(d * n)
    ptr = np.arange(0, R + 1, a.rank)
    Cm = np.zeros((d, n, n))
    Cm[0] = np.eye(n)
    k = KktContext(m, device=0)
    if form == "factored":
        assert k.add_hermitian_factored(F, ptr, None, Cm) == 0
    else:
        A = syn.expand_hermitian_factors(F, ptr, np.ones(R))
        assert k.add_hermitian(A, Cm) == 0
        del A
    k.initialize()
    k.sync()
    W = syn.hermitian_scaling_points(1, n, d, seed=2)[0]
    return k, W, 8.0 * (d * n) * (d * R) if form == "factored" else dense_bytes(n, m, d)


def context(a, form):
    from conex_amd import KktContext
    from conex_amd import synthetic as syn
    rng = np.random.default_rng(1)
    n, m, R = a.n, a.m, a.m * a.rank
    if a.herm:
        k, W, held = hermitian_context(a, form)
    else:
        F = rng.standard_normal((n, R)) / np.sqrt(n)
        ptr = np.arange(0, R + 1, a.rank)
        k = KktContext(m, device=0)
        if form == "factored":
            assert k.add_lmi_factored(F, ptr, None, np.eye(n)) == 0
        else:
            A = np.einsum("aik,bik->iab", F.reshape(n, m, a.rank), F.reshape(n, m, a.rank))
            assert k.add_lmi(A, np.eye(n)) == 0
            del A
        k.initialize()
        k.sync()
        W = syn.scaling_points(1, n, seed=2, scale=0.3)[0]
        held = 8.0 * n * R if form == "factored" else dense_bytes(n, m)
    k.set_W(0, W)
    k.set_y(rng.uniform(-1, 1, k.N) * (0.25 / max(1, m)))
    k.enable_timing(True)
    byt, flops = k.assembly_work()
    info = {"held_bytes": held, "work_flops": flops, "work_bytes": byt}
    if form == "factored":
        assert k.count_factored_lmi() == 1
    return k, W, info


def stage_calls(k, W):
    def prepare():
        k.set_W(0, W)
        k.prepare_step(None, 1.0, 1.0)

    def take():
        prepare()
        k.take_step(0.5, 1.0)

    return {"assembly": k.assemble, "query": lambda: k.weighted_slack_eigenvalues(None, 1.0), "prepare": prepare, "take": take}


def once(k, slot, call):
    for s in STAGES:
        k.kernel_clock(s, reset=True)
    call()
    k.sync()
    n, ms = k.kernel_clock(slot, reset=True)
    assert n == 1, (slot, n)
    return ms * 1e3


def measure(a, forms):
    out = {"n": a.n, "m": a.m, "rank": a.rank, "herm": a.herm, "rounds": a.rounds}
    held = dense_bytes(a.n, a.m, max(a.herm, 1))
    if "dense" in forms and held > a.dense_limit_gb * 2.0 ** 30:
        out["dense_skipped"] = f"the expanded form holds {held / 2.0 ** 30:.1f} GB (limit {a.dense_limit_gb:g})"
        forms = tuple(f for f in forms if f != "dense")
    built = {name: context(a, name) for name in forms}
    calls = {name: stage_calls(k, W) for name, (k, W, _) in built.items()}
    times = {name: {s: [] for s in STAGES} for name in built}
    for r in range(a.warmup + a.rounds):
        for name, (k, _, _) in built.items():  # the forms alternate within a round
            for s in STAGES:
                us = once(k, s, calls[name][s])
                if r >= a.warmup:
                    times[name][s].append(us)
    for name, (k, _, info) in built.items():
        for key, v in info.items():
            out[f"{name}_{key}"] = v
        for s in STAGES:
            out[f"{s}_{name}_us"] = round(float(np.median(times[name][s])), 2)
        k.close()
    return finish(out)


def finish(out):
    if "assembly_factored_us" in out and "assembly_dense_us" in out:
        for s in STAGES:
            out[f"speedup_{s}"] = round(out[f"{s}_dense_us"] / out[f"{s}_factored_us"], 2)
    return out


def child(a, form, parent):
    cmd = [sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--m", str(a.m), "--rank", str(a.rank), "--herm", str(a.herm), "--" + form,
           "--rounds", str(a.rounds), "--warmup", str(a.warmup), "--dense-limit-gb", str(a.dense_limit_gb)]
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
    runs = {"dense": [], "factored": []}
    for pair in range(a.pairs):
        runs["dense"].append(child(a, "dense", True))
        runs["factored"].append(child(a, "factored", False))
        line = {"pair": pair}
        for name in runs:
            for s in STAGES:
                line[f"{s}_{name}_us"] = runs[name][-1][f"{s}_{name}_us"]
        print(json.dumps(finish(line)), flush=True)
    out = {key: runs["factored"][0][key] for key in ("n", "m", "rank", "rounds")}
    out["pairs"] = a.pairs
    for name in runs:
        for key in ("held_bytes", "work_flops", "work_bytes"):
            out[f"{name}_{key}"] = runs[name][0][f"{name}_{key}"]
        for s in STAGES:
            out[f"{s}_{name}_us"] = round(float(np.median([r[f"{s}_{name}_us"] for r in runs[name]])), 2)
    print(json.dumps(finish(out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--m", type=int, default=200)
    ap.add_argument("--rank", type=int, default=1)
    ap.add_argument("--herm", type=int, default=0, choices=(0, 1, 2, 4), help="hyper-complex dimension d of the Hermitian mode (0: real LMI)")
    ap.add_argument("--dense", action="store_true", help="the expanded form only")
    ap.add_argument("--factored", action="store_true", help="the factored form only")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--dense-limit-gb", type=float, default=8.0)
    ap.add_argument("--child-timeout", type=float, default=300.0)
    a = ap.parse_args()
    if a.parent_lib:
        against_parent(a)
        return
    if os.environ.get("CONEX_AMD_LIB"):
        load_other_library()
    forms = ("dense",) if a.dense else ("factored",) if a.factored else ("factored", "dense")
    if a.sweep:
        for a.n, a.m in SWEEP:
            print(json.dumps(measure(a, forms)), flush=True)
    else:
        print(json.dumps(measure(a, forms)), flush=True)


if __name__ == "__main__":
    main()
