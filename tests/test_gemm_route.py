"""csrc/gemm_route.h -- which of the five kernels of gemm_mfma.hip a product runs on and how wide its grid is --
against a table written out independently here, on the CPU: the header is built into a small shared object with g++
and asked about every clause at its edge.  Python integers cannot overflow, so every product below is the
mathematical one.

What the two 2^31 clauses bound (read against the kernels, gemm_mfma.hip MakeDmaLane / gemm_f64_dma / gemm_f64_dma128):
DmaLane::off[], the 32-bit byte offset of a lane's 16-byte chunk from the origin of its 64-row operand image at the
start of a stage.  Everything else in the address (tile origin a0 / b0, stage advance a_step / b_step, batch strides)
is 64-bit pointer arithmetic.
  * k-major image (A under ta, B without tb): off = (rc ld + k) 8, rc <= 63, k <= 30.  The clause 64 ld 8 < 2^31
    bounds it: 63 ld + 30 < 64 ld as soon as ld > 30 (and below that both sides are tiny).
  * m-major image (A without ta, B under tb): off = (k ld + rc) 8 with k <= 31 relative to the stage, rc <= 62.  An
    offset is USED only for k < K - k_lo (the others fetch the zero page, whatever off holds), so a used
    off <= ((min(K, 32) - 1) ld + 62) 8, which is below K ld 8 for ld >= 63.  The clause K ld 8 < 2^31 is therefore
    sufficient (and conservative for K > 32); no admitted call wraps.  gemm_f64_dma128 builds one DmaLane per 64-row
    half with an origin of its own, so the same bounds hold there.
These clauses can only be tested here: on a GPU they need a 2 GiB operand.
"""
import ctypes as C
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ("general", "dma16", "dma32", "dma128x128", "dma128x64")

SRC = r'''
#include "gemm_route.h"
using namespace cxk_host;
// v: M N K lda ldb ldc sA1 sA2 sB1 sB2 a_addr b_addr ta tb accumulate lower_only splits has_ct batch cus forced general
extern "C" int gemm_choose(const long long* v, unsigned* grid_x) {
  GemmShape s;
  s.M = (int)v[0]; s.N = (int)v[1]; s.K = (int)v[2];
  s.lda = v[3]; s.ldb = v[4]; s.ldc = v[5];
  s.sA1 = v[6]; s.sA2 = v[7]; s.sB1 = v[8]; s.sB2 = v[9];
  s.a_addr = (uint64_t)v[10]; s.b_addr = (uint64_t)v[11];
  s.ta = v[12] != 0; s.tb = v[13] != 0; s.accumulate = v[14] != 0; s.lower_only = v[15] != 0;
  s.splits = (int)v[16]; s.has_ct = v[17] != 0; s.batch = (int)v[18];
  GemmModes m;
  m.cus = (int)v[19]; m.forced_tile = (int)v[20]; m.force_general = v[21] != 0;
  const GemmLaunch l = ChooseGemm(s, m);
  *grid_x = l.grid_x;
  switch (l.route) {
    case GemmRoute::kGeneral: return 0;
    case GemmRoute::kDma16: return 1;
    case GemmRoute::kDma32: return 2;
    case GemmRoute::kDma128x128: return 3;
    case GemmRoute::kDma128x64: return 4;
  }
  return -1;
}
'''

ORDER = ("M", "N", "K", "lda", "ldb", "ldc", "sA1", "sA2", "sB1", "sB2", "a_addr", "b_addr", "ta", "tb", "accumulate",
         "lower_only", "splits", "has_ct", "batch", "cus", "forced", "general")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("gemm_route")
    src = d / "gemm_route_test.cc"
    src.write_text(SRC)
    so = d / "libgemm_route_test.so"
    # a bare g++: the header includes nothing of HIP
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "conex_amd", "csrc"), str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    L.gemm_choose.restype = C.c_int
    L.gemm_choose.argtypes = [C.POINTER(C.c_longlong), C.POINTER(C.c_uint)]
    return L


def call(M=128, N=128, K=64, ta=0, tb=0, **kw):
    """a packed, aligned call; the leading dimensions follow the stored shapes unless given"""
    c = dict(M=M, N=N, K=K, ta=ta, tb=tb, lda=(K if ta else M), ldb=(N if tb else K), ldc=M, sA1=0, sA2=0, sB1=0,
             sB2=0, a_addr=4096, b_addr=8192, accumulate=0, lower_only=0, splits=1, has_ct=0, batch=1, cus=256,
             forced=0, general=0)
    c.update(kw)
    return c


def ask(lib, c):
    v = (C.c_longlong * len(ORDER))(*[int(c[k]) for k in ORDER])
    gx = C.c_uint(0)
    r = lib.gemm_choose(v, C.byref(gx))
    return ROUTES[r], gx.value


def cdiv(a, b):
    return -(-a // b)


def table(c):
    """The choice, written out from the description of the kernels (not from the header's text)."""
    M, N, K = c["M"], c["N"], c["K"]
    splits = max(c["splits"], 1)
    t64 = cdiv(M, 64) * cdiv(N, 64)
    # -- can the LDS-DMA kernels fetch this call's operands in aligned 16-byte chunks that stay inside them?
    dma = not c["general"]
    dma = dma and min(M, N, K) >= 2
    dma = dma and all(c[k] % 2 == 0 for k in ("lda", "ldb", "sA1", "sA2", "sB1", "sB2"))
    dma = dma and c["a_addr"] % 16 == 0 and c["b_addr"] % 16 == 0
    a_kmajor, b_kmajor = bool(c["ta"]), not c["tb"]
    if (a_kmajor or b_kmajor) and K % 2:
        dma = False
    if 8 * (64 * c["lda"] if a_kmajor else K * c["lda"]) >= 2 ** 31:
        dma = False
    if 8 * (64 * c["ldb"] if b_kmajor else K * c["ldb"]) >= 2 ** 31:
        dma = False
    if not dma:
        return "general", t64

    # -- a big tile?
    def clean(n, t):
        return n % t == 0 or n % t > t - 16

    def big():
        if c["forced"] == 64:
            return None
        if M <= 32 and N <= 32:
            return None
        if c["accumulate"] and c["splits"] <= 1:
            return None
        if c["forced"] == 128:
            return "dma128x128"
        if c["forced"] == 12864:
            return "dma128x64"
        if M <= 64 or not clean(M, 128):
            return None
        reps = splits * c["batch"] * cdiv(M, 128)
        if N > 64 and clean(N, 128) and reps * cdiv(N, 128) >= c["cus"]:
            return "dma128x128"
        if clean(N, 64) and reps * cdiv(N, 64) >= 2 * c["cus"]:
            return "dma128x64"
        return None

    b = big()
    if b == "dma128x128":
        return b, cdiv(M, 128) * cdiv(N, 128)
    if b == "dma128x64":
        return b, cdiv(M, 128) * cdiv(N, 64)
    per_split = cdiv(cdiv(K, 16), splits) * 16
    tm = cdiv(M, 64)
    gx = tm * (tm + 1) // 2 if c["lower_only"] and M == N else t64
    return ("dma32" if per_split >= 512 else "dma16"), gx


def agree(lib, c, want_route=None):
    got, want = ask(lib, c), table(c)
    assert got == want, (c, got, want)
    if want_route is not None:
        assert got[0] == want_route, (c, got)
    return got


def test_minimum_sizes(lib):
    for M, N, K in itertools.product((1, 2), repeat=3):
        for ta, tb in itertools.product((0, 1), repeat=2):
            # (leading dimensions kept even, so that only the sizes decide)
            c = call(M, N, K, ta, tb, lda=2, ldb=2)
            agree(lib, c, "dma16" if (M, N, K) == (2, 2, 2) else "general")


def test_parity_of_every_leading_dimension_and_stride(lib):
    base = call(70, 66, 34, lda=72, ldb=36, sA1=72 * 34, sB1=36 * 66, sA2=2, sB2=4)
    agree(lib, base, "dma16")
    for k in ("lda", "ldb", "sA1", "sA2", "sB1", "sB2"):
        agree(lib, dict(base, **{k: base[k] + 1}), "general")
        agree(lib, dict(base, **{k: base[k] + 2}), "dma16")
    agree(lib, dict(base, ldc=71), "dma16")      # C is written by plain stores: its parity decides nothing


def test_operand_alignment(lib):
    for a, b in itertools.product((0, 8), repeat=2):
        agree(lib, call(a_addr=4096 + a, b_addr=8192 + b), "dma16" if (a, b) == (0, 0) else "general")


def test_odd_k_needs_both_operands_m_major(lib):
    for ta, tb in itertools.product((0, 1), repeat=2):
        agree(lib, call(64, 64, 33, ta, tb, lda=64, ldb=64), "dma16" if (not ta and tb) else "general")
        agree(lib, call(64, 64, 34, ta, tb, lda=64, ldb=64), "dma16")


def test_byte_offset_limits_of_a_dma_lane(lib):
    lim = 2 ** 31
    # k-major A (ta): 64 lda 8 < 2^31  <=>  lda < 2^22
    for lda, ok in ((2 ** 22 - 2, True), (2 ** 22, False), (2 ** 22 + 2, False)):
        assert (64 * lda * 8 < lim) == ok
        agree(lib, call(64, 64, 32, 1, 0, lda=lda), "dma16" if ok else "general")
    # k-major B (no tb): 64 ldb 8 < 2^31
    for ldb, ok in ((2 ** 22 - 2, True), (2 ** 22, False), (2 ** 22 + 2, False)):
        agree(lib, call(64, 64, 32, 0, 0, ldb=ldb), "dma16" if ok else "general")
    # m-major A (no ta): K lda 8 < 2^31: K = 1024 -> lda < 2^18
    for lda, ok in ((2 ** 18 - 2, True), (2 ** 18, False), (2 ** 18 + 2, False)):
        assert (1024 * lda * 8 < lim) == ok
        agree(lib, call(64, 64, 1024, 0, 0, lda=lda), "dma32" if ok else "general")
    # m-major B (tb): K ldb 8 < 2^31
    for ldb, ok in ((2 ** 18 - 2, True), (2 ** 18, False), (2 ** 18 + 2, False)):
        agree(lib, call(64, 64, 1024, 0, 1, ldb=ldb), "dma32" if ok else "general")
    # the bound itself: the largest byte offset a lane USES stays below 2^31 for every admitted call
    for K in (2, 16, 31, 32, 33, 1024):
        for lda in (K and 2, 62, 64, 2 ** 18 - 2, 2 ** 22 - 2, (lim // 8 - 1) // K // 2 * 2):
            if 8 * K * lda < lim:
                assert ((min(K, 32) - 1) * lda + 62 + 1) * 8 + 8 <= lim     # m-major: rows rc, rc + 1 of column k
            if 8 * 64 * lda < lim and lda >= K:
                assert (63 * lda + 30 + 1) * 8 + 8 <= lim                   # k-major: k, k + 1 of row rc


def test_gram_quadrant_rule(lib):
    # at most 32 x 32: the 64-tile kernel whatever is forced or however many workgroups there are
    for M, N in ((32, 32), (2, 32), (32, 2)):
        for forced in (0, 128, 12864):
            agree(lib, call(M, N, 64, 1, 0, batch=100000, forced=forced), "dma16")
    agree(lib, call(33, 32, 64, 1, 0, lda=64, forced=128), "dma128x128")
    agree(lib, call(32, 33, 64, 1, 0, lda=64, forced=12864), "dma128x64")


def test_accumulating_calls_stay_on_the_small_tile_unless_split(lib):
    big = dict(batch=1000)
    agree(lib, call(128, 128, 64, **big), "dma128x128")
    agree(lib, call(128, 128, 64, accumulate=1, **big), "dma16")
    agree(lib, call(128, 128, 64, accumulate=1, splits=1, forced=128), "dma16")
    agree(lib, call(128, 128, 64, accumulate=1, splits=2, **big), "dma128x128")   # partials: beta is the reduction's
    agree(lib, call(128, 128, 64, accumulate=1, splits=2, forced=12864), "dma128x64")


def test_m_at_most_64(lib):
    agree(lib, call(64, 128, 64, batch=100000), "dma16")
    agree(lib, call(128, 64, 64, batch=100000), "dma128x64")
    agree(lib, call(64, 128, 64, forced=128), "dma128x128")      # (forcing comes before the size rules)


def test_clean_remainders_against_128(lib):
    # remainders 0, 1, 128 - 16, 128 - 15 of M and of N; enough workgroups for either big tile
    for rem, clean in ((0, True), (1, False), (112, False), (113, True)):
        agree(lib, call(128 + rem, 128, 64, lda=128 + rem + (rem & 1), batch=100000), "dma128x128" if clean else "dma16")
    agree(lib, call(128, 128, 64, batch=100000), "dma128x128")
    agree(lib, call(128, 129, 64, batch=100000), "dma16")        # 1: ragged for 128 and for 64
    agree(lib, call(128, 240, 64, batch=100000), "dma16")        # 112 = 64 + 48: ragged for both
    agree(lib, call(128, 241, 64, batch=100000), "dma128x128")   # 113


def test_clean_remainders_against_64(lib):
    """clean(N, 64), the clause of the 128 x 64 tile, on its own: every N here is ragged for 128 (remainder at most
    112) or at most 64 wide, so only the remainder against 64 decides between dma128x64 and dma16."""
    for N, want in ((64, "dma128x64"), (65, "dma16"), (48, "dma16"), (49, "dma128x64"),
                    (192, "dma128x64"), (193, "dma16"), (176, "dma16"), (177, "dma128x64")):
        assert N % 128 <= 112 and N % 128 != 0
        for batch in (512, 100000):     # 512 tiles of one 128-row tile: at 2 cus already for N <= 64
            agree(lib, call(128, N, 64, batch=batch), want)
    # ... and one workgroup short of 2 cus the ragged-but-clean widths stay on the small tile
    agree(lib, call(128, 49, 64, batch=511), "dma16")
    agree(lib, call(128, 177, 64, batch=170), "dma16")           # 170 * 3 = 510
    agree(lib, call(128, 177, 64, batch=171), "dma128x64")       # 513


def test_workgroup_thresholds(lib):
    # 128 x 128: reps tiles >= cus, one below and at, with cus = 256 (reps = splits batch tiles_m)
    agree(lib, call(128, 128, 64, batch=255), "dma16")
    agree(lib, call(128, 128, 64, batch=256), "dma128x128")
    agree(lib, call(256, 256, 64, batch=63), "dma16")        # 63 * 2 * 2 = 252
    agree(lib, call(256, 256, 64, batch=64), "dma128x128")
    agree(lib, call(128, 128, 640, batch=85, splits=3), "dma16")       # 255
    agree(lib, call(128, 128, 640, batch=86, splits=3), "dma128x128")  # 258
    # 128 x 64: >= 2 cus
    agree(lib, call(128, 64, 64, batch=511), "dma16")
    agree(lib, call(128, 64, 64, batch=512), "dma128x64")
    # N = 192 is clean for 64 only
    agree(lib, call(128, 192, 64, batch=170), "dma16")       # 510
    agree(lib, call(128, 192, 64, batch=171), "dma128x64")   # 513
    # another chip
    agree(lib, call(128, 128, 64, batch=128, cus=128), "dma128x128")
    agree(lib, call(128, 128, 64, batch=127, cus=128), "dma16")


def test_stage_depth_switch(lib):
    agree(lib, call(64, 64, 511), "general")   # (odd K with a k-major B)
    agree(lib, call(64, 64, 511, 0, 1, lda=64, ldb=64), "dma32")   # per_split counts whole steps: 32 of 16 = 512
    agree(lib, call(64, 64, 496, 0, 1, lda=64, ldb=64), "dma16")
    agree(lib, call(64, 64, 497, 0, 1, lda=64, ldb=64), "dma32")
    agree(lib, call(64, 64, 512), "dma32")
    agree(lib, call(64, 64, 1024, splits=2), "dma32")
    agree(lib, call(64, 64, 1024, splits=3), "dma16")    # ceil(64 / 3) = 22 steps = 352
    agree(lib, call(64, 64, 1008, splits=2), "dma32")    # 63 steps -> 32 per split = 512
    agree(lib, call(64, 64, 992, splits=2), "dma16")     # 62 steps -> 31 per split = 496


def test_compact_lower_grid(lib):
    for n, tiles in ((2, 1), (64, 1), (65, 2), (128, 2), (129, 3), (257, 5)):
        r, gx = agree(lib, call(n, n, 64, lda=n + (n & 1), lower_only=1, forced=64))
        assert r == "dma16" and gx == tiles * (tiles + 1) // 2
        r, gx = agree(lib, call(n, n, 64, lda=n + (n & 1), forced=64))
        assert gx == tiles * tiles
    # not square: the full grid
    r, gx = agree(lib, call(130, 66, 64, lower_only=1))
    assert (r, gx) == ("dma16", 6)
    # the general kernel and the big tiles have no compact grid
    r, gx = agree(lib, call(129, 129, 64, lower_only=1, general=1))
    assert (r, gx) == ("general", 9)
    r, gx = agree(lib, call(256, 256, 64, lower_only=1, forced=128))
    assert (r, gx) == ("dma128x128", 4)
    r, gx = agree(lib, call(256, 256, 64, lower_only=1, forced=12864))
    assert (r, gx) == ("dma128x64", 8)


def test_forced_tiles(lib):
    for forced, want in ((64, "dma16"), (128, "dma128x128"), (12864, "dma128x64"), (0, "dma128x128"), (7, "dma128x128")):
        agree(lib, call(128, 128, 64, batch=1000, forced=forced), want)
    for forced, want in ((64, "dma16"), (128, "dma128x128"), (12864, "dma128x64"), (0, "dma16")):
        r, gx = agree(lib, call(17, 33, 6, lda=18, ldb=6, forced=forced), want)
        assert gx == 1
    # forcing never makes an ineligible call eligible, and "general" wins over a forced tile
    agree(lib, call(17, 33, 5, lda=18, ldb=6, forced=128), "general")
    agree(lib, call(128, 128, 64, forced=128, general=1), "general")


def test_grid_of_the_general_kernel_and_has_ct(lib):
    r, gx = agree(lib, call(65, 129, 3))
    assert (r, gx) == ("general", 6)
    for ct in (0, 1):
        agree(lib, call(66, 130, 64, has_ct=ct), "dma16")
        agree(lib, call(128, 128, 64, batch=256, has_ct=ct), "dma128x128")


def test_sweep_against_the_table(lib):
    """every clause crossed with the others at a coarser grain"""
    n = 0
    for M, N, K in itertools.product((1, 2, 33, 64, 65, 113, 128, 240, 241), (2, 32, 64, 113, 128, 192), (2, 33, 496, 512)):
        for ta, tb, acc, lower, splits, batch, forced in itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (1, 3),
                                                                           (1, 256, 600), (0, 64, 128, 12864)):
            lda = (K if ta else M)
            ldb = (N if tb else K)
            c = call(M, N, K, ta, tb, lda=lda + (lda & 1), ldb=ldb + (ldb & 1), accumulate=acc, lower_only=lower,
                     splits=splits, batch=batch, forced=forced)
            agree(lib, c)
            n += 1
    assert n > 10000
