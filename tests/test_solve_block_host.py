"""Host-side checks of the block solve's interface (cxk_solve_block / cxk_solve_block_device,
KktContext.solve_block): no GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conex_amd import KktContext, capi
from conex_amd import kkt
from conex_amd.kkt import KktError

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "conex_kkt_hip.h")

CTYPES = {"int": C.c_int, "double*": C.POINTER(C.c_double), "cxk_context*": C.c_void_p}


def header_prototype(name):
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared in conex_kkt_hip.h"
    args = []
    for a in m.group(2).split(","):
        a = re.sub(r"\s+", " ", a.strip())
        if a in ("", "void"):
            continue
        a = re.match(r"^(.*?[\s\*])([A-Za-z_][A-Za-z_0-9]*)$", a).group(1)   # drop the parameter name
        args.append(re.sub(r"\s*\*\s*", "*", a.strip()))
    return m.group(1), args


@pytest.mark.parametrize("name", ["cxk_solve_block", "cxk_solve_block_device"])
def test_both_entry_points_are_declared_with_the_prototypes_of_the_header(name):
    res, args = header_prototype(name)
    assert res == "int" and args == ["cxk_context*", "double*", "int", "int"]
    L = capi.api()                       # declares them (and conex_amd.kkt's table does at load time)
    fn = getattr(L, name)
    assert fn.restype is C.c_int and len(fn.argtypes) == 4
    assert fn.argtypes[0] is C.c_void_p and fn.argtypes[2] is C.c_int and fn.argtypes[3] is C.c_int
    # the block itself: a host pointer to doubles, or a raw device address
    assert fn.argtypes[1] in (C.POINTER(C.c_double), C.c_void_p)
    res_t, arg_t = kkt._SIGNATURES[name]
    assert res_t is C.c_int and len(arg_t) == 4 and arg_t[0] is C.c_void_p
    assert arg_t[1] is (C.POINTER(C.c_double) if name == "cxk_solve_block" else C.c_void_p)
    assert kkt.load_library().cxk_solve_block_chunk_width() >= 16


def host_only(shard=None):
    k = KktContext(2, device=-1)
    k.add_static(np.eye(2), [0, 1])
    if shard:
        k.set_shard(*shard)
    k.initialize()
    return k


def test_host_only_context_refuses_the_block_solve():
    """No CPU fallback: as every numeric call."""
    k = host_only()
    with pytest.raises(KktError, match="no HIP device"):
        k.solve_block(np.ones((2, 3)))
    with pytest.raises(KktError, match="no HIP device"):
        k._check(k.L.cxk_solve_block_device(k.h, C.c_void_p(64), 2, 1), "cxk_solve_block_device")


def test_sharded_context_is_refused_by_name():
    k = host_only(shard=(0, 2))
    with pytest.raises(KktError, match="sharded"):
        k.solve_block(np.ones((2, 3)))
    with pytest.raises(KktError, match="sharded"):
        k._check(k.L.cxk_solve_block_device(k.h, C.c_void_p(64), 2, 1), "cxk_solve_block_device")


class NoSolve:
    """The library without its block solve: the structure getters (the system size) stay."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name.startswith("cxk_solve_block"):
            raise AssertionError(f"{name} was called before the arguments were checked")
        return getattr(self._lib, name)


@pytest.mark.parametrize("bad", [np.ones((3, 2)), np.ones((2, 0)), np.ones((2, 2, 2)), np.ones(3), np.float64(1.0),
                                 np.ones((2, 2), dtype=complex), np.array([["a", "b"], ["c", "d"]])])
def test_argument_checks_raise_before_the_library_is_called(bad):
    k = host_only()
    k.L = NoSolve(k.L)
    with pytest.raises(ValueError, match="solve_block"):
        k.solve_block(bad)


def test_a_one_dimensional_input_reaches_the_library_as_one_column():
    k = host_only()
    seen = []

    class Spy(NoSolve):
        def __getattr__(self, name):
            if name == "cxk_solve_block":
                return lambda h, ptr, ld, nrhs: seen.append((ld, nrhs)) or 0
            return getattr(self._lib, name)
    k.L = Spy(k.L)
    x = k.solve_block(np.array([1.0, 2.0]))
    assert seen == [(2, 1)] and x.shape == (2,)
    X = k.solve_block(np.ones((2, 5), order="C"))
    assert seen[-1] == (2, 5) and X.shape == (2, 5) and X.flags.f_contiguous
