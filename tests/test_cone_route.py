"""csrc/cone_route.h -- which set of kernels a constraint runs on (Choose), how a group of matrix inequalities
assembles its Schur complement (ChooseLmiAssembly) and the dynamic-LDS formulas both are admitted by -- against a table
written out independently here, on the CPU: the header is built into a small shared object with g++ and asked about
the product of every mode value with the shape edges.  A refusal is compared by its exact text.  Python integers
cannot overflow, so every product below is the mathematical one.
"""
import ctypes as C
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INT_MAX = 2 ** 31 - 1
LDS = 160 * 1024 - 512   # kLdsLimit
LMI, LINEAR, SOC, STATIC, QUAD, OCT = 0, 1, 2, 3, 4, 5   # conex_kkt_hip.h

ROUTES = ("linear-lds", "linear-tiled", "linear-sparse", "soc-lds", "soc-streamed", "soc-sparse", "quad-lds",
          "quad-streamed", "lmi-dense", "lmi-sparse", "lmi-factored", "static", "oct")
ASSEMBLIES = ("generic", "mfma", "gemm")

# the enumerators by name: the shim translates them, so that the header may order them as it likes
SRC = r'''
#include "cone_route.h"
using namespace cxk_host;
static int Code(ConeRoute r) {
  switch (r) {
    case ConeRoute::kLinearLds: return 0;
    case ConeRoute::kLinearTiled: return 1;
    case ConeRoute::kLinearSparse: return 2;
    case ConeRoute::kSocLds: return 3;
    case ConeRoute::kSocStreamed: return 4;
    case ConeRoute::kSocSparse: return 5;
    case ConeRoute::kQuadLds: return 6;
    case ConeRoute::kQuadStreamed: return 7;
    case ConeRoute::kLmiDense: return 8;
    case ConeRoute::kLmiSparse: return 9;
    case ConeRoute::kLmiFactored: return 10;
    case ConeRoute::kStatic: return 11;
    case ConeRoute::kOct: return 12;
  }
  return -1;
}
static const ConeRoute kRoutes[13] = {
    ConeRoute::kLinearLds, ConeRoute::kLinearTiled, ConeRoute::kLinearSparse, ConeRoute::kSocLds, ConeRoute::kSocStreamed,
    ConeRoute::kSocSparse, ConeRoute::kQuadLds, ConeRoute::kQuadStreamed, ConeRoute::kLmiDense, ConeRoute::kLmiSparse,
    ConeRoute::kLmiFactored, ConeRoute::kStatic, ConeRoute::kOct};
// shape: type n m herm_d symmetric csr_only factored has_q nnz_fits_int nnz sum_nnz_sq longest_column mfma_supports sparse_pays
// modes: streamed_cones tiled_linear streamed_quadratic sparse_linear sparse_soc sparse_lmi tiled_min_work quad_min_work
//        linear_ratio soc_ratio
extern "C" int cone_choose(const double* s, const double* md, const char** refusal) {
  ConeShape sh;
  sh.type = (int)s[0]; sh.n = (int)s[1]; sh.m = (int)s[2]; sh.herm_d = (int)s[3];
  sh.symmetric = s[4] != 0; sh.csr_only = s[5] != 0; sh.factored = s[6] != 0; sh.has_q = s[7] != 0;
  sh.nnz_fits_int = s[8] != 0; sh.nnz = s[9]; sh.sum_nnz_sq = s[10]; sh.longest_column = (int)s[11];
  sh.mfma_supports = s[12] != 0; sh.sparse_pays = s[13] != 0;
  RouteModes m;
  m.streamed_cones = md[0] != 0; m.tiled_linear = (int)md[1]; m.streamed_quadratic = (int)md[2];
  m.sparse_linear = (int)md[3]; m.sparse_soc = (int)md[4]; m.sparse_lmi = (int)md[5];
  m.tiled_linear_min_work = (long long)md[6]; m.streamed_quadratic_min_work = (long long)md[7];
  m.sparse_linear_min_ratio = md[8]; m.sparse_soc_min_ratio = md[9];
  const RouteChoice c = Choose(sh, m);
  *refusal = c.refusal;
  return c.refusal ? -1 : Code(c.route);
}
extern "C" int cone_assembly(int route, int n, int m, unsigned long long count, int literal, int mfma_supports,
                             int schur_generic, int gemm_min_n, int* large) {
  const LmiAssemblyChoice a = ChooseLmiAssembly(kRoutes[route], n, m, (size_t)count, literal != 0, mfma_supports != 0,
                                                schur_generic != 0, gemm_min_n);
  *large = a.large;
  switch (a.assembly) {
    case LmiAssembly::kGeneric: return 0;
    case LmiAssembly::kMfma: return 1;
    case LmiAssembly::kGemm: return 2;
  }
  return -1;
}
extern "C" unsigned long long cone_lds(int which, int n, int m, int staged) {
  switch (which) {
    case 0: return LmiGenericLds(n);
    case 1: return LmiPrepareLds(n, m);
    case 2: return LmiTakeLds(n);
    case 3: return SocSchurLds(n, m, staged != 0);
    case 4: return SocPrepareLds(n, m);
    case 5: return SocTakeLds(n);
    case 6: return QuadSchurLds(n, m);
    case 7: return QuadPrepareLds(n, m);
    default: return QuadTakeLds(n);
  }
}
extern "C" void cone_defaults(double* out) {
  const RouteModes m;
  out[0] = (double)kLdsLimit; out[1] = kLinearLdsMaxVars; out[2] = (double)m.tiled_linear_min_work;
  out[3] = (double)m.streamed_quadratic_min_work; out[4] = m.sparse_linear_min_ratio; out[5] = m.sparse_soc_min_ratio;
  out[6] = (double)kSparseLinearMinWork; out[7] = kSparseLinearMaxColumn; out[8] = (double)kSparseSocMinWork;
}
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("cone_route")
    src = d / "cone_route_test.cc"
    src.write_text(SRC)
    so = d / "libcone_route_test.so"
    # a bare g++: no HIP; the one header cone_route.h includes is the C header that names the constraint types
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "conex_amd", "csrc"), str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    L.cone_choose.restype = C.c_int
    L.cone_choose.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_char_p)]
    L.cone_assembly.restype = C.c_int
    L.cone_assembly.argtypes = [C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.POINTER(C.c_int)]
    L.cone_lds.restype = C.c_ulonglong
    L.cone_lds.argtypes = [C.c_int] * 4
    L.cone_defaults.restype = None
    L.cone_defaults.argtypes = [C.POINTER(C.c_double)]
    return L


SHAPE_KEYS = ("type", "n", "m", "herm_d", "symmetric", "csr_only", "factored", "has_q", "nnz_fits_int", "nnz",
              "sum_nnz_sq", "longest_column", "mfma_supports", "sparse_pays")
MODE_KEYS = ("streamed_cones", "tiled_linear", "streamed_quadratic", "sparse_linear", "sparse_soc", "sparse_lmi",
             "tiled_linear_min_work", "streamed_quadratic_min_work", "sparse_linear_min_ratio", "sparse_soc_min_ratio")


def shape(type_, n, m, **kw):
    s = dict(type=type_, n=n, m=m, herm_d=0, symmetric=True, csr_only=False, factored=False, has_q=False,
             nnz_fits_int=True, nnz=0, sum_nnz_sq=0, longest_column=0, mfma_supports=False, sparse_pays=False)
    assert set(kw) <= set(s), kw
    s.update(kw)
    return s


def modes(**kw):
    md = dict(streamed_cones=False, tiled_linear=-1, streamed_quadratic=0, sparse_linear=0, sparse_soc=0, sparse_lmi=-1,
              tiled_linear_min_work=16_384_000, streamed_quadratic_min_work=1288, sparse_linear_min_ratio=7.8,
              sparse_soc_min_ratio=4.04)
    assert set(kw) <= set(md), kw
    md.update(kw)
    return md


def ask(lib, s, md):
    """('route', name) or ('refusal', text), as the header answers."""
    a = (C.c_double * len(SHAPE_KEYS))(*[float(s[k]) for k in SHAPE_KEYS])
    b = (C.c_double * len(MODE_KEYS))(*[float(md[k]) for k in MODE_KEYS])
    why = C.c_char_p()
    r = lib.cone_choose(a, b, C.byref(why))
    if r < 0:
        assert why.value is not None
        return ("refusal", why.value.decode())
    assert why.value is None  # never both
    return ("route", ROUTES[r])


# ------------------------------------------------------------------------------------ the table
def lmi_lds_resident(n, m):
    return 8 * 5 * n * n <= LDS and 8 * (3 * n * n + 6 * n + 2 * (n // 2 + 2) + m + 8) <= LDS


R_LINEAR_CSR = ("a linear block added by cxk_add_linear_csr has no dense matrix and can only take the sparse route "
                "(cxk_set_sparse_linear / CXK_SPARSE_LINEAR, which is 0)")
R_LINEAR_NNZ = "a sparse linear block with more than 2^31 nonzeros is not supported"
R_LINEAR_SPARSE_MM = "a sparse linear block whose variables x variables Schur block exceeds the int range is not supported"
R_TILED_ENTRIES = "a tiled linear block whose rows x variables entries exceed the int range is not supported"
R_TILED_MM = "a tiled linear block whose variables x variables Schur block exceeds the int range is not supported"
R_LINEAR_LDS = ("a linear block over more than 4096 variables does not fit the LDS route's kernels: it needs the tiled "
                "route (cxk_set_tiled_linear / CXK_TILED_LINEAR, which was set to 0)")
R_SOC_CSR = ("a second-order cone added by cxk_add_soc_csr has no dense matrix and can only take the sparse route "
             "(cxk_set_sparse_soc / CXK_SPARSE_SOC, which is 0)")
R_SOC_NNZ = "a sparse second-order cone with more than 2^31 nonzeros is not supported"
R_SOC_SPARSE_MM = "a sparse second-order cone whose variables x variables Schur block exceeds the int range is not supported"
R_SOC_STREAM_ENTRIES = ("a streamed second-order cone whose (dimension + 1) x variables entries exceed the int range is not "
                        "supported")
R_SOC_STREAM_MM = "a streamed second-order cone whose variables x variables Schur block exceeds the int range is not supported"
R_SOC_IMAGE = "a second-order cone whose (dimension + 1) x (variables + 2) image exceeds LDS (160 KB) is not supported"
R_SOC_STEPS = ("a second-order cone whose step kernels need more than the 163 328 B of LDS (four vectors of dimension + 1) is "
               "not supported")
R_QUAD_ENTRIES = "a streamed quadratic cone whose (dimension + 1) x variables entries exceed the int range is not supported"
R_QUAD_MM = "a streamed quadratic cone whose variables x variables Schur block exceeds the int range is not supported"
R_QUAD_Q = "a streamed quadratic cone whose inner-product matrix has more than 2^31 entries is not supported"
R_QUAD_LDS = ("a quadratic cone whose step kernels need more than the 163 328 B of LDS (variables + four vectors of "
              "dimension + 1) is not supported")
R_LMI_LITERAL = ("non-symmetric LMI data beyond the LDS-resident orders is not supported: "
                 "the large-order kernels use tr(W A_i W A_j) = tr(P_i P_j), which needs A_i = A_i^T")


def table(s, md):
    """The route cxk_finalize has always chosen, or the first refusal it has always raised."""
    n, m, t = s["n"], s["m"], s["type"]
    if t == LINEAR:
        mode, tiled_mode = md["sparse_linear"], md["tiled_linear"]
        if s["csr_only"] and mode == 0:
            return ("refusal", R_LINEAR_CSR)
        measured = mode != 0 and not s["csr_only"]
        countable = s["nnz_fits_int"] or not measured
        if not countable and mode == 1:
            return ("refusal", R_LINEAR_NNZ)
        sparse = s["csr_only"] or mode == 1
        if mode == -1 and not s["csr_only"] and tiled_mode < 0 and countable:
            sparse = (md["sparse_linear_min_ratio"] * s["sum_nnz_sq"] <= n * m * m and n * m * m >= 8_192_000
                      and s["longest_column"] <= 2048)
        if sparse:
            return ("refusal", R_LINEAR_SPARSE_MM) if m * m > INT_MAX else ("route", "linear-sparse")
        tiled = tiled_mode != 0 if tiled_mode >= 0 else (m > 4096 or n * m * m >= md["tiled_linear_min_work"])
        if tiled:
            if n * max(m, 1) > INT_MAX - 1024:
                return ("refusal", R_TILED_ENTRIES)
            return ("refusal", R_TILED_MM) if m * m > INT_MAX else ("route", "linear-tiled")
        return ("refusal", R_LINEAR_LDS) if m > 4096 else ("route", "linear-lds")
    if t == SOC:
        mode = md["sparse_soc"]
        if s["csr_only"] and mode == 0:
            return ("refusal", R_SOC_CSR)
        measured = mode != 0 and not s["csr_only"]
        countable = s["nnz_fits_int"] or not measured
        if not countable and mode == 1:
            return ("refusal", R_SOC_NNZ)
        dense_ok = (n + 1) * max(m, 1) <= INT_MAX - 1024
        sparse = s["csr_only"] or mode == 1
        if mode == -1 and not s["csr_only"] and countable:
            sparse = not dense_ok or (md["sparse_soc_min_ratio"] * s["nnz"] <= (n + 1) * m
                                      and (n + 1) * m * m >= 2_984_242)
        if sparse:
            return ("refusal", R_SOC_SPARSE_MM) if m * m > INT_MAX else ("route", "soc-sparse")
        image_fits = 8 * (n + 1) * (m + 2) <= LDS
        steps_fit = 8 * 4 * (n + 1) <= LDS and 8 * (m + 3 * (n + 1)) <= LDS
        if md["streamed_cones"] and not (image_fits and steps_fit):
            if not dense_ok:
                return ("refusal", R_SOC_STREAM_ENTRIES)
            return ("refusal", R_SOC_STREAM_MM) if m * m > INT_MAX else ("route", "soc-streamed")
        if not image_fits:
            return ("refusal", R_SOC_IMAGE)
        return ("route", "soc-lds") if steps_fit else ("refusal", R_SOC_STEPS)
    if t == QUAD:
        mode = md["streamed_quadratic"]
        fits = 8 * (m + 4 * (n + 1)) <= LDS and 8 * (2 * n + m + 4) <= LDS and 8 * 3 * (n + 1) <= LDS
        work = (n * n if s["has_q"] else 0) + (n + 1) * m
        streamed = mode != 0 if mode >= 0 else (not fits or work >= md["streamed_quadratic_min_work"])
        if streamed:
            if (n + 1) * max(m, 1) > INT_MAX - 1024:
                return ("refusal", R_QUAD_ENTRIES)
            if m * m > INT_MAX:
                return ("refusal", R_QUAD_MM)
            return ("refusal", R_QUAD_Q) if s["has_q"] and n * n > INT_MAX else ("route", "quad-streamed")
        return ("route", "quad-lds") if fits else ("refusal", R_QUAD_LDS)
    if t == LMI:
        if s["factored"]:
            return ("route", "lmi-factored")
        sparse = md["sparse_lmi"] != 0 if md["sparse_lmi"] >= 0 else s["sparse_pays"]
        if n > 65535:
            sparse = False
        if not s["symmetric"]:
            if not lmi_lds_resident(n, m):
                return ("refusal", R_LMI_LITERAL)
            sparse = False
        return ("route", "lmi-sparse" if sparse else "lmi-dense")
    return ("route", "oct" if t == OCT else "static")


def assembly_table(route, n, m, count, literal, mfma_supports, schur_generic, gemm_min_n):
    """(large, assembly) as UploadGroup has always decided them."""
    if route == "lmi-factored":
        return True, "generic"
    large = not lmi_lds_resident(n, m)
    sparse = route == "lmi-sparse"
    mfma = not sparse and not large and not literal and not schur_generic and mfma_supports
    gemm = not sparse and not literal and (large or (not mfma and n >= gemm_min_n
                                                     and count * 2 * (m + 1) * n * n * 8 <= 8 << 30))
    assert not (mfma and gemm)
    return large, "mfma" if mfma else "gemm" if gemm else "generic"


# ------------------------------------------------------------------------------------ the walks
def check(lib, s, md, seen=None):
    got, want = ask(lib, s, md), table(s, md)
    assert got == want, (s, md, got, want)
    if seen is not None:
        seen.add(want)
    return want


def linear_edges():
    out = [dict(n=3, m=m) for m in (0, 1, 4096, 4097, 46340, 46341)]
    # rows m^2 one below and at the tiled threshold, as 4000 x 64 and as one column
    out += [dict(n=4000, m=64), dict(n=3999, m=64), dict(n=16_383_999, m=1), dict(n=16_384_000, m=1)]
    # rows x max(m, 1) at and past INT_MAX - 1024
    out += [dict(n=INT_MAX - 1024, m=1), dict(n=INT_MAX - 1023, m=1), dict(n=INT_MAX - 1024, m=0), dict(n=INT_MAX - 1023, m=0),
            dict(n=(INT_MAX - 1023) // 4097 + 1, m=4097)]
    # rows m^2 / sum nnz^2 one side and the other of 7.8 (8 192 000 / 7.8 = 1 050 256.4)
    out += [dict(n=2000, m=64, sum_nnz_sq=1_050_256, nnz=2000, longest_column=32),
            dict(n=2000, m=64, sum_nnz_sq=1_050_257, nnz=2000, longest_column=32)]
    # rows m^2 at and below the sparse floor, one nonzero per row
    out += [dict(n=2000, m=64, sum_nnz_sq=2000, nnz=2000, longest_column=32),
            dict(n=1999, m=64, sum_nnz_sq=1999, nnz=1999, longest_column=32)]
    # above the tiled threshold and sparse enough: the sparse route goes first
    out += [dict(n=4000, m=64, sum_nnz_sq=4000, nnz=4000, longest_column=63)]
    # the longest column
    out += [dict(n=4000, m=64, sum_nnz_sq=4000, nnz=4000, longest_column=c) for c in (2048, 2049)]
    # more nonzeros than an int counts
    out += [dict(n=INT_MAX - 1024, m=2, nnz_fits_int=False, nnz=2 ** 31), dict(n=3, m=46341, nnz_fits_int=False, nnz=2 ** 31)]
    return out


def test_linear_blocks(lib):
    seen = set()
    for sparse_mode, tiled_mode, csr in itertools.product((-1, 0, 1), (-1, 0, 1), (False, True)):
        md = modes(sparse_linear=sparse_mode, tiled_linear=tiled_mode)
        for e in linear_edges():
            if csr and not e.get("nnz_fits_int", True):
                continue  # (cxk_add_linear_csr takes int pointers: such a block cannot be added)
            check(lib, shape(LINEAR, csr_only=csr, **e), md, seen)
    # a moved threshold and a moved ratio
    check(lib, shape(LINEAR, 100, 10), modes(tiled_linear_min_work=10_000), seen)
    check(lib, shape(LINEAR, 100, 10), modes(tiled_linear_min_work=10_001), seen)
    for ratio in (1.0, 2.0, 2.1):
        check(lib, shape(LINEAR, 2000, 64, sum_nnz_sq=4_096_000, longest_column=2000),
              modes(sparse_linear=-1, sparse_linear_min_ratio=ratio), seen)
    assert seen == {("route", "linear-lds"), ("route", "linear-tiled"), ("route", "linear-sparse")} | {
        ("refusal", r) for r in (R_LINEAR_CSR, R_LINEAR_NNZ, R_LINEAR_SPARSE_MM, R_TILED_ENTRIES, R_TILED_MM, R_LINEAR_LDS)}


def soc_edges():
    out = [dict(n=3, m=2, nnz=8)]
    # (n + 1)(m + 2) at 20 416 doubles and one row past (320 x 64)
    out += [dict(n=318, m=62, nnz=319 * 62), dict(n=319, m=62, nnz=320 * 62)]
    # the step kernels' four vectors: n + 1 at 5104 and 5105 with one variable
    out += [dict(n=5103, m=1, nnz=5104), dict(n=5104, m=1, nnz=5105)]
    # len m / nnz one side and the other of 4.04 (2048 x 64: 131 072 / 4.04 = 32 443.6)
    out += [dict(n=2047, m=64, nnz=32_443), dict(n=2047, m=64, nnz=32_444)]
    # len m^2 at and below the floor of 2 984 242
    out += [dict(n=2_984_241, m=1, nnz=10), dict(n=2_984_240, m=1, nnz=10)]
    # (n + 1) x m past the int range, sparse enough and not
    out += [dict(n=2 ** 20 - 1, m=2048, nnz=2 ** 21), dict(n=2 ** 20 - 1, m=2048, nnz=2 ** 30),
            dict(n=INT_MAX - 1024 - 1, m=0), dict(n=INT_MAX - 1024, m=0)]
    out += [dict(n=3, m=46341, nnz=10), dict(n=3, m=46340, nnz=10)]
    out += [dict(n=2 ** 20 - 1, m=2048, nnz_fits_int=False, nnz=2 ** 31)]
    return out


def test_second_order_cones(lib):
    seen = set()
    for sparse_mode, streamed, csr in itertools.product((-1, 0, 1), (False, True), (False, True)):
        md = modes(sparse_soc=sparse_mode, streamed_cones=streamed)
        for e in soc_edges():
            if csr and not e.get("nnz_fits_int", True):
                continue
            check(lib, shape(SOC, csr_only=csr, **e), md, seen)
    for ratio in (1.0, 2.0, 2.1):
        check(lib, shape(SOC, 2047, 64, nnz=65_536), modes(sparse_soc=-1, streamed_cones=True, sparse_soc_min_ratio=ratio), seen)
    assert seen == {("route", "soc-lds"), ("route", "soc-streamed"), ("route", "soc-sparse")} | {
        ("refusal", r) for r in (R_SOC_CSR, R_SOC_NNZ, R_SOC_SPARSE_MM, R_SOC_STREAM_ENTRIES, R_SOC_STREAM_MM, R_SOC_IMAGE,
                                 R_SOC_STEPS)}


def test_quadratic_cones(lib):
    seen = set()
    edges = [dict(n=3, m=2)]
    # the LDS edge of QuadPrepareLds: m + 4 (n + 1) at 20 416 doubles and past
    edges += [dict(n=5103, m=0), dict(n=5104, m=0), dict(n=5102, m=4), dict(n=5102, m=5)]
    # work 1288 (n = 32 with Q over m = 8) and one column less
    edges += [dict(n=32, m=8), dict(n=32, m=7)]
    # the three int-range refusals
    edges += [dict(n=2 ** 20 - 1, m=2048), dict(n=3, m=46341), dict(n=46341, m=1), dict(n=46340, m=1)]
    for mode, has_q in itertools.product((-1, 0, 1), (False, True)):
        for e in edges:
            check(lib, shape(QUAD, has_q=has_q, **e), modes(streamed_quadratic=mode), seen)
    check(lib, shape(QUAD, 3, 2), modes(streamed_quadratic=-1, streamed_quadratic_min_work=8), seen)
    check(lib, shape(QUAD, 3, 2), modes(streamed_quadratic=-1, streamed_quadratic_min_work=9), seen)
    assert seen == {("route", "quad-lds"), ("route", "quad-streamed")} | {
        ("refusal", r) for r in (R_QUAD_ENTRIES, R_QUAD_MM, R_QUAD_Q, R_QUAD_LDS)}


LMI_ORDERS = (8, 9, 63, 64, 65535, 65536)


def test_matrix_inequalities(lib):
    seen = set()
    for sparse_lmi, symmetric, factored, mfma, pays, n in itertools.product((-1, 0, 1), (True, False), (False, True),
                                                                             (False, True), (False, True), LMI_ORDERS):
        check(lib, shape(LMI, n, 3, symmetric=symmetric, factored=factored, mfma_supports=mfma, sparse_pays=pays),
              modes(sparse_lmi=sparse_lmi), seen)
    assert seen == {("route", "lmi-dense"), ("route", "lmi-sparse"), ("route", "lmi-factored"), ("refusal", R_LMI_LITERAL)}
    assert lmi_lds_resident(63, 3) and not lmi_lds_resident(64, 3)  # (the orders walked straddle the edge)


def ask_assembly(lib, route, n, m, count, literal, mfma, generic, min_n):
    large = C.c_int(-1)
    a = lib.cone_assembly(ROUTES.index(route), n, m, count, int(literal), int(mfma), int(generic), min_n, C.byref(large))
    return bool(large.value), ASSEMBLIES[a]


def test_the_assembly_of_a_group_of_matrix_inequalities(lib):
    seen = set()
    # the 8 GB bound on the GEMM assembly's work space of a group: one member either side
    per_member = 2 * (1 + 1) * 63 * 63 * 8
    edge = (8 << 30) // per_member
    assert edge * per_member <= 8 << 30 < (edge + 1) * per_member
    counts = (1, 1000, edge, edge + 1)
    for route, generic, literal, mfma, n, count, min_n in itertools.product(
            ("lmi-dense", "lmi-sparse", "lmi-factored"), (False, True), (False, True), (False, True), LMI_ORDERS, counts,
            (9, 10, 64)):
        if literal and (route != "lmi-dense" or not lmi_lds_resident(n, 1)):
            continue  # (Choose refuses non-symmetric data beyond LDS, and keeps it off the other two routes)
        got = ask_assembly(lib, route, n, 1, count, literal, mfma, generic, min_n)
        want = assembly_table(route, n, 1, count, literal, mfma, generic, min_n)
        assert got == want, (route, generic, literal, mfma, n, count, min_n, got, want)
        seen.add(want)
    assert seen == {(False, "generic"), (False, "mfma"), (False, "gemm"), (True, "gemm"), (True, "generic")}


def test_the_lds_formulas_in_size_t(lib):
    """Orders at which the products pass the int range (5 n^2 from 20 725, 4 n^2 from 23 171, n^2 itself at 46 341)."""
    for n in (3, 20, 20725, 23171, 46341):
        for m in (0, 7, 46341):
            want = (8 * 4 * n * n, 8 * (3 * n * n + 6 * n + 2 * (n // 2 + 2) + m + 8), 8 * 5 * n * n, None,
                    8 * (m + 3 * (n + 1)), 8 * 4 * (n + 1), 8 * (2 * n + m + 4), 8 * (m + 4 * (n + 1)), 8 * 3 * (n + 1))
            for which, w in enumerate(want):
                if w is not None:
                    assert lib.cone_lds(which, n, m, 0) == w, (which, n, m)
            assert lib.cone_lds(3, n, m, 0) == 8 * (n + 1) * (m + 2)
            assert lib.cone_lds(3, n, m, 1) == 8 * (n + 1) * (2 * m + 4)


def test_the_constants(lib):
    d = (C.c_double * 9)()
    lib.cone_defaults(d)
    assert list(d) == [LDS, 4096, 16_384_000, 1288, 7.8, 4.04, 8_192_000, 2048, 2_984_242]
    assert list(modes().values())[6:] == list(d)[2:6]


# What tests/test_gpu_every_route.py builds in one context (64 variables, streamed cones on, tiled linear, sparse
# linear, sparse second-order and streamed quadratic at automatic), by the name it gives the constraint there:
# the shape as GroupConstraints measures it, and the route the device test asserts through the counters.
EVERY_ROUTE_MODES = dict(streamed_cones=True, tiled_linear=-1, sparse_linear=-1, sparse_soc=-1, streamed_quadratic=-1)
EVERY_ROUTE = {
    "linear-lds": (shape(LINEAR, 3, 2, nnz=6, sum_nnz_sq=12, longest_column=3), "linear-lds"),
    "linear-tiled": (shape(LINEAR, 4000, 64, nnz=4000 * 64, sum_nnz_sq=4000 * 64 * 64, longest_column=4000), "linear-tiled"),
    "linear-sparse": (shape(LINEAR, 2000, 64, nnz=2000, sum_nnz_sq=2000, longest_column=32), "linear-sparse"),
    "soc-lds": (shape(SOC, 3, 2, nnz=8, sum_nnz_sq=16, longest_column=4), "soc-lds"),
    "soc-streamed": (shape(SOC, 319, 62, nnz=320 * 62, sum_nnz_sq=320 * 62 * 62, longest_column=320), "soc-streamed"),
    "soc-sparse": (shape(SOC, 5, 3, csr_only=True), "soc-sparse"),
    "quad-lds": (shape(QUAD, 3, 2), "quad-lds"),
    "quad-streamed": (shape(QUAD, 32, 8, has_q=True), "quad-streamed"),
    "lmi-mfma": (shape(LMI, 8, 2, mfma_supports=True), "lmi-dense"),
    "lmi-literal": (shape(LMI, 3, 2, symmetric=False, mfma_supports=True), "lmi-dense"),
    "lmi-gemm": (shape(LMI, 25, 2), "lmi-dense"),
    "lmi-large": (shape(LMI, 64, 2), "lmi-dense"),
    "lmi-sparse": (shape(LMI, 10, 2, mfma_supports=True, sparse_pays=True), "lmi-sparse"),
    "lmi-factored": (shape(LMI, 6, 3, factored=True), "lmi-factored"),
    "static": (shape(STATIC, 0, 3), "static"),
    "oct": (shape(OCT, 2, 2, herm_d=8), "oct"),
}
EVERY_ROUTE_ASSEMBLY = {"lmi-mfma": (False, "mfma"), "lmi-literal": (False, "generic"), "lmi-gemm": (False, "gemm"),
                        "lmi-large": (True, "gemm"), "lmi-sparse": (False, "generic"), "lmi-factored": (True, "generic")}


def test_the_shapes_of_the_device_test_reach_their_routes(lib):
    md = modes(**EVERY_ROUTE_MODES)
    for name, (s, route) in EVERY_ROUTE.items():
        assert check(lib, s, md) == ("route", route), name
    assert {r for _, r in EVERY_ROUTE.values()} == set(ROUTES)
    for name, want in EVERY_ROUTE_ASSEMBLY.items():
        s, route = EVERY_ROUTE[name]
        got = ask_assembly(lib, route, s["n"], s["m"], 1, not s["symmetric"], s["mfma_supports"], False, 9)
        assert got == want == assembly_table(route, s["n"], s["m"], 1, not s["symmetric"], s["mfma_supports"], False, 9), name


def test_the_header_is_plain_cxx():
    """No HIP, no I/O, no allocation: nothing included to do any of them with."""
    with open(os.path.join(ROOT, "conex_amd", "csrc", "cone_route.h")) as f:
        includes = [l.split()[1] for l in f if l.startswith("#include")]
    assert includes == ["<climits>", "<cstddef>", "<cstdint>", '"../../include/conex_kkt_hip.h"']
    with open(os.path.join(ROOT, "include", "conex_kkt_hip.h")) as f:
        assert not [l for l in f if l.startswith("#include")]  # (the C header that names the constraint types)
