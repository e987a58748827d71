"""The Newton-step entry points in every call order the KKT interface allows (include/conex_kkt_hip.h).

Most tests call in one order: W, b, assemble, factor, solve.  The hot path does not: the triple launch
(cxk_factor_solve_triple_async) leaves three solutions, the direction for the barrier parameter the device
selects is combined from them later (cxk_newton_direction_device_mu, often deferred into PrepareStep), and
host-side flags decide whether those shortcuts still hold.  Here one KktContext is driven through call
sequences and every y it returns is held against a float64 reference of the SAME state:

  * the residual vectors AW, AQc of the latest assembly and the dense KKT matrix come from the oracle
    (oracle/, kept in step through set_W / set_identity and assembled where the context assembles);
  * the matrix whose factor the context holds is tracked separately (cxk_set_slab can put back the slab of
    an earlier assembly), b is the latest cxk_set_cost;
  * a solve of cb b + cq AQc + cw AW is numpy's dense solve in float64; relative error <= 1e-10 (the
    north-star bound of the parity tests).  A stale or mis-scaled y is off by O(1).

The barrier parameter is selected with lb == ub in the random sequences, so the model knows it exactly;
the directed cases run the real rule and read it back from cxk_prepare_take_step_device_mu.
"""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
from conex_amd import KktContext, synthetic as syn

pytestmark = pytest.mark.gpu

TOL = 1e-10
BS, CS = 0.9, 0.8
OTHER_SCALINGS = (0.5, 1.3)    # another ratio bs : cs than (BS, CS)


def _program(kind):
    """(problem, build kind, scaling points, second scaling points, rankK)."""
    if kind == "lmi":          # small LMI tree: the whole tree in one launch, the triple launch applies
        prob = syn.lmi_problem(K=40, n=20, m=20, branching=4, overlap=5, seed=5)
        return prob, "lmi", list(syn.scaling_points(40, 20, seed=10)), list(syn.scaling_points(40, 20, seed=11)), 800
    if kind == "mixed":        # (test_gpu_step_tail.py's mixed program)
        prob = syn.mixed_problem(K=46, herm_every=(4, 7), branching=4, overlap=3)
        return (prob, "mixed", syn.mixed_scaling_points(prob, seed=32), syn.mixed_scaling_points(prob, seed=33),
                300)
    if kind == "soc":
        prob = syn.soc_problem(K=60, dim=6, m=5, overlap=2, tree=4)
        return prob, "soc", list(syn.soc_scaling_points(60, 6, seed=3)), list(syn.soc_scaling_points(60, 6, seed=4)), 120
    raise ValueError(kind)


CONFIGS = {  # name: (program, environment at context creation)
    "lmi": ("lmi", {}),
    "lmi-no-fused-tree": ("lmi", {"CXK_NO_FUSED_TREE": "1"}),
    "lmi-no-y-deferral": ("lmi", {"CXK_NO_Y_DEFERRAL": "1"}),
    "mixed": ("mixed", {}),
    "soc": ("soc", {}),
}


def _context(prob, build_kind, env):
    """The switches are read once, at cxk_create / cxk_finalize: set them around the build only."""
    saved = {v: os.environ.get(v) for v in env}
    os.environ.update(env)
    try:
        return syn.build(KktContext, prob, build_kind, device=0)
    finally:
        for v, old in saved.items():
            if old is None:
                os.environ.pop(v, None)
            else:
                os.environ[v] = old


def _rel(y, want):
    return np.linalg.norm(y - want) / np.linalg.norm(want)


class Model:
    """One device context, its oracle twin, and what the context must hold after each call."""

    def __init__(self, config):
        kind, env = CONFIGS[config]
        self.config = config
        prob, build_kind, Wa, Wb, self.rankK = _program(kind)
        self.k = _context(prob, build_kind, env)
        self.o = syn.build(ol.Program, prob, build_kind)
        self.L, self.h = self.k.L, self.k.h
        self.pools = (Wa, Wb)
        rng = np.random.default_rng(7)
        b0 = np.asarray(prob["b"], dtype=np.float64)
        self.costs = [b0, b0 + 0.5 * np.linalg.norm(b0) / np.sqrt(len(b0)) * rng.standard_normal(len(b0)),
                      -0.7 * b0]
        self.device_mu = self.L.cxk_device_mu_supported(self.h) == 1
        self.triple_capable = None    # known after the first assemble (cxk_triple_supported)
        self.log = []

    # ------------------------------------------------------------ bookkeeping
    def where(self):
        return f"[{self.config}] {self.tag}: " + " -> ".join(self.log)

    def _sys(self):
        """The oracle assembled from the current W: dense KKT matrix and residual vectors."""
        self.o.assemble()
        AW, AQc, _ = self.o.residuals()
        return {"K": self.o.kkt_matrix(), "AW": AW, "AQc": AQc}

    def _solve(self, cb, cq, cw):
        assert self.mat is not None and self.vec is not None, self.where()
        rhs = cb * self.b + cq * self.vec["AQc"] + cw * self.vec["AW"]
        return np.linalg.solve(self.mat["K"], rhs)

    def _check_y(self, what="get_y"):
        y = self.k.get_y()
        err = _rel(y, self.y_exp)
        assert err <= TOL, f"{what}: relative error {err:.3e} {self.where()}"

    def _put_W(self, i, w):
        self.W[i] = w
        self.k.set_W(i, w)
        self.o.set_W(i, w)

    def _restore_W(self):
        """PrepareStep / TakeStep change W on the device (not under test here): put the model's W back."""
        for i, w in enumerate(self.W):
            self.k.set_W(i, w)
        self.log.append("restore_W")

    # ------------------------------------------------------------ the calls
    def reset(self, tag):
        """A known state: W from the first pool, the first cost, one full KKT solve."""
        self.tag = tag
        self.log = []
        self.W = [None] * self.k.K
        for i, w in enumerate(self.pools[0]):
            self._put_W(i, w)
        self.b = self.costs[0]
        self.k.set_cost(self.b)
        self.mu_k = None      # the barrier parameter on the device, when the model knows it
        self.captured = []    # (slab, system) of the latest assemblies
        self.last = None
        self.call("kkt_solve", 0.7, BS, CS)
        self.log = ["reset"]

    def call(self, name, *args):
        self.log.append(name + (repr(tuple(round(a, 4) if isinstance(a, float) else a for a in args)) if args else ""))
        getattr(self, "c_" + name)(*args)
        self.last = name

    def c_set_cost(self, j):
        self.b = self.costs[j]
        self.k.set_cost(self.b)

    def c_set_W(self, idx, pool):
        for i in idx:
            self._put_W(i, self.pools[pool][i])

    def c_set_identity(self):
        self.k.set_identity()
        self.o.set_identity()
        self.W = [np.asarray(self.k.get_W(i)).copy() for i in range(self.k.K)]

    def c_set_slab(self):       # a round trip: the slab as it is
        self.k.set_slab(self.k.slab())

    def c_restore_slab(self, j):  # the slab of an earlier assembly: an unfactored matrix
        S, sys = self.captured[j]
        self.k.set_slab(S)
        self.mat, self.slab_state = sys, "assembled"

    def c_assemble(self):
        # (the slab of this assembly is kept for c_restore_slab: the second assemble is the one that counts,
        # its gather still waits for the factorization that follows)
        self.k.assemble()
        S = self.k.slab().copy()
        self.k.assemble()
        self.vec = self.mat = self._sys()
        self.captured = (self.captured + [(S, self.mat)])[-2:]
        self.slab_state = "assembled"
        if self.triple_capable is None:
            self.triple_capable = self.L.cxk_triple_supported(self.h) == 1

    def c_factor(self):
        assert self.k.factor() == 1, self.where()
        self.slab_state = "factored"
        self.y_exp = None     # (a factorization alone says nothing about y)

    def c_kkt_solve(self, kk, bs, cs):
        self.k.kkt_solve_async(kk, bs, cs)
        assert self.k.sync() == 1, self.where()
        self.vec = self.mat = self._sys()
        self.slab_state = "factored"
        self.y_exp = self._solve(kk * bs, kk * cs, -2.0)

    def c_sync(self):
        assert self.k.sync() == 1, self.where()

    def c_factor_solve(self, cb, cq, cw):
        self.k.factor_solve_async(cb, cq, cw)
        self.slab_state = "factored"
        self.y_exp = self._solve(cb, cq, cw)

    def c_factor_direction(self, kk, bs, cs):
        self.k.factor_direction_async(kk, bs, cs)
        self.slab_state = "factored"
        self.y_exp = self._solve(kk * bs, kk * cs, -2.0)

    def c_triple(self, bs, cs):
        assert self.L.cxk_triple_supported(self.h) == 1, self.where()
        self.k._check(self.L.cxk_factor_solve_triple_async(self.h, bs, cs), "cxk_factor_solve_triple_async")
        self.slab_state = "factored"
        self.y_exp = self._solve(-bs, cs, 0.0)

    def c_solve_rhs(self, cb, cq, cw):
        self.k.solve_rhs(cb, cq, cw)
        self.y_exp = self._solve(cb, cq, cw)

    def c_select_mu(self, kk):
        # lb == ub: whatever the rule computes from the eigenvalues, the device holds exactly kk
        self.k._check(self.L.cxk_select_mu_async(self.h, CS, 1.0, self.rankK, 0.3, kk, kk), "cxk_select_mu_async")
        self.mu_k = kk

    def c_direction_device_mu(self, bs, cs):
        self.k._check(self.L.cxk_newton_direction_device_mu(self.h, bs, cs), "cxk_newton_direction_device_mu")
        self.y_exp = self._solve(self.mu_k * bs, self.mu_k * cs, -2.0)

    def c_get_y(self):
        self._check_y()

    def c_prepare_step(self):
        self.k.prepare_step(None, 0.7 * CS)
        self._check_y("get_y behind prepare_step")
        self._restore_W()

    def c_prepare_take_step(self):
        self.k.prepare_take_step(None, 0.7 * CS)
        self._check_y("get_y behind prepare_take_step")
        self._restore_W()

    def c_prepare_take_step_device_mu(self):
        info, took, inv = np.zeros(2), C.c_int(0), C.c_double(0)
        self.k._check(self.L.cxk_prepare_take_step_device_mu(self.h, CS, 1.0, ol.dp(info), C.byref(took),
                                                             C.byref(inv)), "cxk_prepare_take_step_device_mu")
        assert inv.value == self.mu_k, (inv.value, self.mu_k, self.where())
        self._check_y("get_y behind prepare_take_step_device_mu")
        self._restore_W()

    # ------------------------------------------------------------ legal next calls
    def legal(self, rng):
        """(weight, name, args) of every call whose CXK_DEMAND preconditions the current state meets."""
        K = self.k.K
        factored = self.slab_state == "factored"
        have_y = self.y_exp is not None
        out = [(1, "set_cost", (int(rng.integers(len(self.costs))),)),
               (1, "set_W", (sorted(rng.choice(K, size=max(1, K // 4), replace=False).tolist()), int(rng.integers(2)))),
               (0.3, "set_identity", ()),
               (0.5, "set_slab", ()),
               (3, "assemble", ()),
               (1, "kkt_solve", (float(rng.choice([0.5, 0.7, 1.1])), BS, CS)),
               (0.5, "sync", ())]
        if self.captured:
            out.append((0.5, "restore_slab", (int(rng.integers(len(self.captured))),)))
        if self.slab_state == "assembled":
            out += [(1, "factor", ()), (1, "factor_solve", (-BS, CS, 0.0)),
                    (1, "factor_direction", (float(rng.choice([0.6, 0.9])), BS, CS))]
        if self.last == "assemble" and self.triple_capable:
            out.append((12, "triple", (BS, CS)))
        if factored:
            out.append((1, "solve_rhs", (float(rng.choice([-BS, 0.4])), CS, float(rng.choice([0.0, -1.0])))))
        if self.device_mu and have_y:
            out.append((3 if self.last == "triple" else 1, "select_mu", (float(rng.choice([0.6, 0.75, 1.2])),)))
        if self.device_mu and self.mu_k is not None and factored:
            scal = (BS, CS) if rng.random() < 0.7 else OTHER_SCALINGS
            out.append((6 if self.last == "select_mu" else 1, "direction_device_mu", scal))
        if have_y:
            out += [(2, "get_y", ()), (0.5, "prepare_step", ()), (0.5, "prepare_take_step", ())]
            if self.device_mu and self.mu_k is not None:
                out.append((3 if self.last == "direction_device_mu" else 0.5, "prepare_take_step_device_mu", ()))
        return out

    def run_random(self, seed, length):
        rng = np.random.default_rng(seed)
        for _ in range(length):
            cands = self.legal(rng)
            w = np.array([c[0] for c in cands], dtype=float)
            _, name, args = cands[rng.choice(len(cands), p=w / w.sum())]
            self.call(name, *args)
        if self.y_exp is not None:
            self.call("get_y")


_MODELS = {}


def _model(config):
    if config not in _MODELS:
        _MODELS[config] = Model(config)
    return _MODELS[config]


SEEDS = list(range(1000, 1024))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_random_call_sequences_against_the_reference(config, seed):
    m = _model(config)
    m.reset(f"seed {seed}")
    m.run_random(seed, 8 + seed % 13)


# ------------------------------------------------------------------ directed: triple, X, direction, read y
def _other_slab(m):
    """The slab of an assembly from the second pool of W (an unfactored matrix other than the current one),
    captured without disturbing the model's residual vectors: the current W is put back and assembled again."""
    idx = list(range(m.k.K))
    m.call("set_W", idx, 1)
    m.call("assemble")
    m.call("set_slab")                  # (flushes the deferred gather: the slab of that assembly)
    S, sys = m.captured[-1]
    m.call("set_W", idx, 0)
    return S, sys


DIRECTED = ["set_cost", "set_W", "set_identity", "set_slab", "factor", "solve_rhs", "factor_solve_async",
            "other_scalings"]


@pytest.mark.parametrize("x", DIRECTED)
@pytest.mark.parametrize("config", ["lmi", "lmi-no-y-deferral"])
def test_direction_behind_the_triple_launch_after_an_intervening_call(config, x):
    """assemble, triple launch, mu selection (the real rule), X, the device-mu direction, PrepareStep: the
    direction must be a fresh solve with the inputs as X left them and the mu the device chose (read back from
    cxk_prepare_take_step_device_mu).  factor / factor_solve_async refactor the slab of ANOTHER assembly
    (put back by cxk_set_slab): the factor behind the three solutions is then gone."""
    m = _model(config)
    m.reset(f"directed {x}")
    other = _other_slab(m) if x in ("factor", "factor_solve_async") else None
    m.call("assemble")
    assert m.triple_capable, m.where()
    m.call("triple", BS, CS)
    m.k._check(m.L.cxk_select_mu_async(m.h, CS, 1.0, m.rankK, 0.3, 1e-8, 1e9), "cxk_select_mu_async")
    m.log.append("select_mu(rule)")
    bs, cs = BS, CS
    if x == "set_cost":
        m.call("set_cost", 1)
    elif x == "set_W":
        m.call("set_W", list(range(0, m.k.K, 3)), 1)
    elif x == "set_identity":
        m.call("set_identity")
    elif x == "set_slab":
        m.call("set_slab")
    elif x == "factor":
        m.k.set_slab(other[0])
        m.mat = other[1]
        m.log.append("restore_slab(other)")
        m.call("factor")
    elif x == "solve_rhs":
        m.call("solve_rhs", 0.4, CS, -1.0)
    elif x == "factor_solve_async":
        m.k.set_slab(other[0])
        m.mat = other[1]
        m.log.append("restore_slab(other)")
        m.call("factor_solve", -BS, CS, 0.0)
    elif x == "other_scalings":
        bs, cs = OTHER_SCALINGS
    m.k._check(m.L.cxk_newton_direction_device_mu(m.h, bs, cs), "cxk_newton_direction_device_mu")
    m.log.append(f"direction_device_mu{(bs, cs)}")
    assert m.L.cxk_step_scalars_async(m.h) == 0
    info, took, inv = np.zeros(2), C.c_int(0), C.c_double(0)
    m.k._check(m.L.cxk_prepare_take_step_device_mu(m.h, CS, 1.0, ol.dp(info), C.byref(took), C.byref(inv)),
               "cxk_prepare_take_step_device_mu")
    m.log.append("prepare_take_step_device_mu")
    kk = inv.value
    assert 1e-8 <= kk <= 1e9, m.where()
    m.y_exp = m._solve(kk * bs, kk * cs, -2.0)
    m._check_y(f"direction for mu {kk:.6g}")
    m._restore_W()


@pytest.mark.parametrize("scalings", [(BS, CS), OTHER_SCALINGS])
def test_steady_state_order_still_combines_the_three_solutions(scalings):
    """The normal order -- assemble, triple, select_mu, direction, PrepareStep -- keeps the shortcut: no
    solve-only sweep goes out (kernel clock CXK_CLOCK_SOLVE), and the direction formed inside PrepareStep is the
    bits of newton_from_three's launch (CXK_NO_Y_DEFERRAL).  Other scalings than the triple launch's are one
    sweep per iteration instead."""
    res = []
    for m in (_model("lmi"), _model("lmi-no-y-deferral")):
        m.reset(f"steady state {scalings}")
        m.k.enable_timing(True)
        for it in range(2):
            m.call("assemble")
            m.call("triple", BS, CS)
            m.call("select_mu", 0.75)
            m.call("direction_device_mu", *scalings)
            assert m.L.cxk_step_scalars_async(m.h) == 0
            m.call("prepare_take_step_device_mu")
        m.call("sync")
        m.k.enable_timing(False)
        sweeps, _ = m.k.kernel_clock("solve")
        assert sweeps == (0 if scalings == (BS, CS) else 2), (sweeps, m.where())
        res.append(m.k.get_y())
    assert np.array_equal(res[0], res[1])


# ------------------------------------------------------------------ time-outs through the debug hook
TIMEOUT_ORDERS = ["solve_sweep", "triple_direction", "select_mu_prepare"]


@pytest.mark.parametrize("order", TIMEOUT_ORDERS)
def test_a_timed_out_wait_with_work_queued_behind_it_is_never_a_silent_wrong_y(order):
    """cxk_debug_force_fused_timeout only raises the host-visible flag (no device wait runs out).  Then one of
    the orders below is queued and cxk_sync asked: it may redo and report success only with y equal to the
    reference for the LAST requested right-hand side; otherwise it reports failure together with
    cxk_fused_tree_timed_out.  Either way the context then solves correctly on the level kernels."""
    m = Model("lmi")          # (a context of its own: the fall-back to the level kernels is for good)
    m.reset(f"timeout {order}")
    assert m.k.fused_tree(), m.where()
    if order == "solve_sweep":
        m.k.kkt_solve_async(0.6, BS, CS)       # (same W: the model's system stands)
        m.log.append("kkt_solve_async(0.6)")
        m.k.debug_force_fused_timeout()
        m.log.append("force_timeout")
        m.call("solve_rhs", 0.4, CS, -1.0)     # the last requested right-hand side
    elif order == "triple_direction":
        m.call("assemble")
        m.call("triple", BS, CS)
        m.k.debug_force_fused_timeout()
        m.log.append("force_timeout")
        m.call("select_mu", 0.75)
        m.call("direction_device_mu", BS, CS)
    else:
        m.k.kkt_solve_async(0.6, BS, CS)
        m.log.append("kkt_solve_async(0.6)")
        m.y_exp = m._solve(0.6 * BS, 0.6 * CS, -2.0)
        m.k.debug_force_fused_timeout()
        m.log.append("force_timeout")
        m.call("select_mu", 0.75)
        info, took, inv = np.zeros(2), C.c_int(0), C.c_double(0)
        m.k._check(m.L.cxk_prepare_take_step_device_mu(m.h, CS, 1.0, ol.dp(info), C.byref(took), C.byref(inv)),
                   "cxk_prepare_take_step_device_mu")
        m.log.append("prepare_take_step_device_mu")
    ok = m.k.sync()
    m.log.append(f"sync -> {ok}")
    if ok:
        m._check_y("y behind a time-out reported as success")
    else:
        assert m.k.fused_tree_timed_out(), f"failure without the time-out signal {m.where()}"
    assert not m.k.fused_tree(), m.where()
    m._restore_W()
    m.call("kkt_solve", 0.7, BS, CS)
    m.call("get_y")
    oko, yo = m.o.kkt_solve(m.b, 0.7, BS, CS)
    assert oko == 1 and _rel(m.k.get_y(), yo) <= TOL, m.where()
