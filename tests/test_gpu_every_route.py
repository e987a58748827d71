"""One context that holds one constraint on every route of cone_route.h (every enumerator of ConeRoute, and for the
dense matrix inequalities every assembly and the large-order kernels), under the automatic modes.

The counters say that every constraint reached its route -- tests/test_cone_route.py holds the same shapes in its
table (EVERY_ROUTE), so the choice is checked there on the CPU and cannot be passed here on another route.  Then every
constraint is finalized alone in a context that forces its route, and after assembly, PrepareStep and TakeStep the
constraint in the mixed context is compared with itself alone: its Schur block, its row of step_info and its W are the
same bits (its kernels do not know who else is there; what they compute is checked against references by the tests
of each route).  Every shape is the smallest that reaches its route.
"""
import numpy as np
import pytest

import test_gpu_cone_kernel_matrix as km
from conex_amd import KktContext
from conex_amd import synthetic as syn
from test_cone_route import EVERY_ROUTE
from test_gpu_lmi_factored import same_bits

pytestmark = pytest.mark.gpu

NUM_VARS = 64
C_WEIGHT = 1.0


def lmi(rng, n, m, symmetric=True):
    A = np.stack([syn.random_sym(rng, n) if symmetric else rng.uniform(-1, 1, (n, n)) for _ in range(m)])
    return A, np.eye(n), syn.scaling_points(1, n, seed=int(rng.integers(1 << 30)))[0]


def constraints():
    """[(name, add(k) -> id, W or None, settings(k) that force the route in a context of its own, environment)]"""
    rng = np.random.default_rng(2031)
    out = []

    def cone(kind, n, m, extra=None):
        return km.make_cone(kind, n, m, extra, "well", rng)

    def var(m, at):
        return list(range(at, at + m))

    ll = cone("lin", 3, 2)
    out.append(("linear-lds", lambda k: k.add_linear(ll["A"], ll["c"], var(2, 0)), ll["W"],
                lambda k: (k.set_tiled_linear(0), k.set_sparse_linear(0))))
    lt = cone("lin", 4000, 64)
    out.append(("linear-tiled", lambda k: k.add_linear(lt["A"], lt["c"], var(64, 0)), lt["W"],
                lambda k: (k.set_tiled_linear(1), k.set_sparse_linear(0))))
    ls = cone("lin", 2000, 64)
    ls["A"] = np.zeros((2000, 64))
    ls["A"][np.arange(2000), np.arange(2000) % 64] = rng.uniform(0.5, 1.0, 2000)  # one nonzero per row
    out.append(("linear-sparse", lambda k: k.add_linear(ls["A"], ls["c"], var(64, 0)), ls["W"],
                lambda k: k.set_sparse_linear(1)))
    sl = cone("soc", 3, 2)
    out.append(("soc-lds", lambda k: k.add_soc(sl["A"], sl["c"], var(2, 1)), sl["W"], lambda k: k.set_sparse_soc(0)))
    st = cone("soc", 319, 62)
    st["A"], st["c"] = km.soc_data(319, 62)  # one past the LDS edge and below the sparse floor
    out.append(("soc-streamed", lambda k: k.add_soc(st["A"], st["c"], var(62, 2)), st["W"],
                lambda k: (k.set_streamed_cones(), k.set_sparse_soc(0))))
    ss = cone("soc", 5, 3)
    rows, cols = np.nonzero(np.ones((6, 3)))
    out.append(("soc-sparse", lambda k: k.add_soc_csr(3 * np.arange(7), cols, ss["A"][rows, cols], ss["c"], var(3, 3)),
                ss["W"], lambda k: k.set_sparse_soc(1)))
    ql = cone("quad", 3, 2)
    out.append(("quad-lds", lambda k: k.add_quadratic(None, ql["A"], ql["c"], var(2, 4)), ql["W"],
                lambda k: k.set_streamed_quadratic(0)))
    qs = cone("quad", 32, 8, "Q")
    out.append(("quad-streamed", lambda k: k.add_quadratic(qs["Q"], qs["A"], qs["c"], var(8, 5)), qs["W"],
                lambda k: k.set_streamed_quadratic(1)))
    for name, n, at, symmetric in (("lmi-mfma", 8, 6, True), ("lmi-literal", 3, 7, False), ("lmi-gemm", 25, 8, True),
                                   ("lmi-large", 64, 9, True)):
        A, Cm, W = lmi(rng, n, 2, symmetric)
        out.append((name, lambda k, A=A, Cm=Cm, at=at: k.add_lmi(A, Cm, var(2, at)), W, None))
    A, Cm, W = lmi(rng, 10, 2)
    A[:] = 0.0
    A[0, 2, 2] = A[1, 7, 7] = 1.0  # one nonzero each: automatic mode evaluates the constraint from its nonzeros
    out.append(("lmi-sparse", lambda k: k.add_lmi(A, Cm, var(2, 10)), W, None, {"CXK_SPARSE_LMI": "1"}))
    F = rng.standard_normal((6, 4))
    out.append(("lmi-factored", lambda k: k.add_lmi_factored(F, [0, 1, 3, 4], None, np.eye(6), var(3, 11)),
                syn.scaling_points(1, 6, seed=7)[0], None))
    sb = cone("static", 0, 3)
    out.append(("static", lambda k: k.add_static(sb["G"], var(3, 12)), None, None))
    oc = cone("oct", 2, 2)
    out.append(("oct", lambda k: k.add_hermitian(oc["A"], oc["C"], var(2, 13)), oc["W"], None))
    return [c if len(c) == 5 else c + ({},) for c in out]


def build(rows, settings, monkeypatch, env):
    with monkeypatch.context() as mp:
        for key, value in env.items():
            mp.setenv(key, value)
        k = KktContext(NUM_VARS, device=0)
        settings(k)
        ids = {name: add(k) for name, add, _, _, _ in rows}
        assert sorted(ids.values()) == list(range(len(rows)))
        k.initialize()
    for name, _, W, _, _ in rows:
        if W is not None:
            k.set_W(ids[name], W)
    return k, ids


def run_stages(k, ids, y):
    """{name: [Schur block, AW, AQc, scalars, row of step_info, W after the step]}"""
    k.assemble()
    out = {name: list(k.constraint_schur(i)) for name, i in ids.items()}
    k.prepare_step(y, C_WEIGHT, 1.0)
    info = k.step_info()
    k.take_step(0.5, 1.0)
    for name, i in ids.items():
        out[name] += [info[i]] + ([k.get_W(i)] if name != "static" else [])
    return out


def test_schur_blocks_come_back_as_full_symmetric_squares(monkeypatch):
    """On the device a Schur block's contract is its lower triangle, and the matrix-inequality routes write nothing else
    (Arena::G, lmi_types.h); constraint_schur hands out that triangle mirrored.  On every route: finite, exactly
    symmetric, and not a triangle with zeros (or whatever the allocation held) above it."""
    rows = constraints()
    for row in rows:
        name, _, _, settings, env = row
        k, ids = build([row], settings or (lambda k: None), monkeypatch, env)
        k.assemble()
        G = k.constraint_schur(ids[name])[0]
        assert G.shape[0] == G.shape[1] >= 2, name
        assert np.all(np.isfinite(G)), name
        assert same_bits(G, G.T.copy()), name
        if name.startswith("lmi-"):  # the routes that leave the upper triangle unwritten on the device
            assert np.any(np.triu(G, 1) != 0.0), name


def test_one_constraint_on_every_route_is_what_it_is_alone(monkeypatch):
    rows = constraints()
    assert [r[0] for r in rows] == list(EVERY_ROUTE)  # (the shapes test_cone_route.py holds in its table)

    def automatic(k):
        k.set_streamed_cones(True)
        k.set_tiled_linear(-1)
        k.set_sparse_linear(-1)
        k.set_sparse_soc(-1)
        k.set_streamed_quadratic(-1)

    k, ids = build(rows, automatic, monkeypatch, {})
    assert (k.count_tiled_linear(), k.count_sparse_linear(), k.count_streamed_cones(), k.count_sparse_soc(),
            k.count_streamed_quadratic()) == (1, 1, 1, 1, 1)
    assert k.count_sparse_lmi() == 1 and k.count_factored_lmi() == 1
    # literal, (rows kernel: none), MFMA, GEMM (order 25, and order 64 on the large-order kernels), sparse
    assert [k.count_lmi_kernel(w) for w in range(5)] == [1, 0, 1, 2, 1]
    assert k.lmi_kernels(ids["lmi-gemm"])["take"].startswith("lmi_take_step_rows")
    assert k.lmi_kernels(ids["lmi-large"])["take"].startswith("LmiLargeTakeStep")
    assert k.lmi_kernels(ids["lmi-literal"])["schur"] == "lmi_schur_generic literal"

    y = 0.01 * np.random.default_rng(2032).uniform(-1, 1, NUM_VARS)
    mixed = run_stages(k, ids, y)
    for row in rows:
        name, _, _, settings, env = row
        alone, ids0 = build([row], settings or (lambda k: None), monkeypatch, env)
        assert ids0[name] == 0 and alone.K == 1
        one = run_stages(alone, ids0, y)[name]
        assert len(one) == len(mixed[name])
        for what, a, b in zip(("G", "AW", "AQc", "scalars", "step_info", "W"), mixed[name], one):
            assert np.all(np.isfinite(a)), (name, what)
            assert same_bits(a, b), (name, what)
