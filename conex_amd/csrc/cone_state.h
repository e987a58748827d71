// The host-side state of a group of equal-shaped constraints: DevBuf (an owned device allocation), then what every
// route has (Group) around one by-value state struct per cone family.  A family's struct is read and written in its own
// unit only -- lin in cone_linear.hip, soc in cone_soc.hip, quad in cone_quad.hip, lmi in cone_lmi.hip (cone_units.h) --
// but for:
//   kkt_cone_launch.hip  GroupConstraints writes the group key (lmi.literal, quad.has_q, quad.sq.on / has_s / rank, quad.sa.on,
//                        lmi.f.R, lmi.sa.on);
//                        UploadDenseData reads lmi.assembly; UploadGroup reads quad.sq.on and quad.sa.on; StepTailOk reads lmi.large and lmi.literal,
//                        TakeStepFromDeviceOk lmi.large
//   MakeVec              (cone_linear.hip) hands lin.T2 to every vector cone's kernels, the other families' included
// Host code only, no device code.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>
#include <vector>

#include "cone_route.h"  // ConeRoute, LmiAssembly

// A function only the units of the cxk_* path call in one another, or a type only they hold: not part of the library's
// dynamic symbols (a type's inline members and the templates instantiated on it follow it).
#define CXK_LOCAL __attribute__((visibility("hidden")))

namespace cxk_host {

// Move-only: a copy would free the allocation twice (std::vector<Group> moves its groups when it grows).
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) {
    o.p = nullptr;
    o.n = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      n = o.n;
      o.p = nullptr;
      o.n = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  // `zeroed`: the code relies on the initial zeros (slots that are never written but read).
  // Everything else is scratch that must be written before it is read: with CXK_DEBUG_FILL_NAN=1
  // in the environment such buffers start as NaN (all-ones bytes), so that a read of unwritten
  // memory shows up in the results instead of passing by luck (diagnostic runs of the test suite).
  hipError_t alloc(size_t count, bool zeroed = false) {
    release();
    n = count;
    if (count == 0) count = 1;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T));
    static const bool nan_fill = [] {
      const char* v = getenv("CXK_DEBUG_FILL_NAN");
      return v && atoi(v) != 0;
    }();
    // the fill runs on the null stream, kernels on the context's stream, which may be
    // non-blocking (no implicit ordering with the null stream): wait for it on the host
    if (e == hipSuccess) e = hipMemset(p, (nan_fill && !zeroed) ? 0xFF : 0, count * sizeof(T));
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    return e;
  }
  hipError_t upload(const std::vector<T>& v) {
    hipError_t e = alloc(v.size());
    if (e != hipSuccess || v.empty()) return e;
    e = hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    return e;
  }
};
static_assert(!std::is_copy_constructible<DevBuf<double>>::value && !std::is_copy_assignable<DevBuf<double>>::value,
              "a copied DevBuf frees its allocation twice");
static_assert(std::is_nothrow_move_constructible<DevBuf<double>>::value && std::is_nothrow_move_assignable<DevBuf<double>>::value,
              "std::vector moves its elements on growth only when the move cannot throw");

// ---- shared by two families, each through the same functions of cone_linear.hip

// The work space of the Gram product Gf = alpha WA' WA (AllocGramWorkspace, LaunchGramLower): tiled linear blocks
// (kLinearTiled, len = n) and streamed second-order cones (kSocStreamed, len = n + 1).
struct CXK_LOCAL GramWs {
  DevBuf<double> WA;    // the scaled copy of A, count x len x m: diag(w) A of a linear block, WA of a second-order cone
  DevBuf<double> Gf;    // the Gram product's output, count x m x m
  DevBuf<double> part;  // its split partials (`splits` of them; empty without a split)
  int splits = 1;       // K splits of the product (SocStreamSplits, or CXK_GRAM_SPLITS)
};

// Every member's nonzeros by rows (col, val) and by columns (crow, cval) from eptr[member] on, the pointers of its rows
// and columns relative to that (UploadSparseNonzeros): sparse linear blocks (kLinearSparse, rows = n) and sparse
// second-order cones (kSocSparse, rows = n + 1).  Such a group has no dense A.
struct CXK_LOCAL NonzeroLists {
  DevBuf<int> eptr, rowptr, col, colptr, crow;
  DevBuf<double> val, cval;
};

// ---- one struct per family

// Linear blocks: cone_linear.hip.
struct CXK_LOCAL LinearState {
  DevBuf<double> T2;  // every CXK_LINEAR group, whatever its route: the second temporary (VecGroup::T2)
  // the tiled route (kLinearTiled, cxk_set_tiled_linear): the kernels of kernels_linear_tiled.hip.h
  GramWs gram;
  // kLinearTiled and kLinearSparse: four doubles per row tile
  DevBuf<double> tile_part;
  // the sparse route (kLinearSparse, cxk_set_sparse_linear): the kernels of kernels_linear_sparse.hip.h
  NonzeroLists nz;
};

// Second-order cones: cone_soc.hip.
struct CXK_LOCAL SocState {
  // cones beyond LDS (kSocStreamed, cxk_set_streamed_cones): the kernels of kernels_soc_stream.hip.h
  GramWs gram;
  // kSocStreamed: s, Q(s) c, the slack: three vectors per cone (MakeSocStream).  kSocSparse: s, ms, u = A' w and
  // (det w, w . c) (MakeSocSparse lays it out)
  DevBuf<double> vec;
  DevBuf<double> det;  // kSocStreamed: det(s) per cone
  int stages = 0;      // kSocStreamed, CXK_SOC_STREAM_STAGES: 1 / 2 = the assembly stops after the vectors / the apply stage (timing runs)
  // the sparse route (kSocSparse, cxk_set_sparse_soc): the kernels of kernels_soc_sparse.hip.h.  No dense A, no WA, no
  // GEMM output.
  NonzeroLists nz;
  // kSocSparse: the constants H = A' J A, h = A' J c, z = c' J c of every member (formed on the device at finalize;
  // MakeSocSparse lays them out)
  DevBuf<double> consts;
};

// Quadratic cones: cone_quad.hip.
struct CXK_LOCAL QuadState {
  bool has_q = false;        // the members carry an inner-product matrix Q
  DevBuf<double> Q, Gram, S;  // Q, A1' Q A1, the state kept between PrepareStep and TakeStep
  // cones held in HBM (kQuadStreamed, cxk_set_streamed_quadratic): the kernels of kernels_quad_stream.hip.h
  int splits = 1;       // column splits of the products with Q (QuadStreamSplits; 1 where Q is the identity)
  DevBuf<double> part;  // the split partials of those products
  DevBuf<double> vec;   // every vector and scalar of the work space (MakeQuadStream lays it out)
  // kQuadStreamed with Q = S + F diag(sigma) F' held by its parts (cxk_add_quadratic_structured): the kernels of
  // kernels_quad_structured.hip.h make the products with Q.  No Q: `has_q` is set, Q stays empty, splits is 1.
  // Members agree on rank and on having S (the group key); their nonzeros are concatenated.
  struct Structured {
    bool on = false, has_s = false;
    int rank = 0;
    int lanes = 1;  // lanes per row of S (cone_route.h: QuadCsrLanes, or CXK_QUAD_CSR_LANES)
    int segs = 1;   // row segments of the factor dots (QuadFactorSegments)
    DevBuf<long long> rowptr;  // count x (n + 1), absolute positions in col / val
    DevBuf<int> col;
    DevBuf<double> val, F, sigma;
    DevBuf<double> tpart;  // count x 2 x rank x segs
  } sq;
  // kQuadStreamed with A held by its nonzeros (cxk_add_quadratic_csr), whatever the form of Q: the kernels of
  // kernels_quad_sparse.hip.h stand where the route reads A.  Group::A stays empty; row 0 of A is kept dense.  Members
  // have their own patterns (nz.eptr); u = A1' Q c1 in `vec` is made once at cxk_finalize.
  struct SparseA {
    bool on = false;
    NonzeroLists nz;
    DevBuf<double> a0;  // count x m
  } sa;
};

// Matrix inequalities: cone_lmi.hip.
struct CXK_LOCAL LmiState {
  // how the Schur complement is assembled: the batched MFMA GEMM pipeline always when `large`, and for LDS-resident
  // shapes from order 9 up without a register-kernel instance, where it measured 1.5-3.3x faster than the LDS kernel
  // (cone_route.h: ChooseLmiAssembly; PlanLmiGroup sets it)
  LmiAssembly assembly = LmiAssembly::kGeneric;
  bool literal = false;  // non-symmetric data: literal kernels only
  // orders beyond the LDS-resident kernels: HBM-resident matrices + MFMA GEMM pipeline
  bool large = false;
  // lmi_schur_mfma launches of this group so far: an odd one walks each workgroup's constraints backwards, so
  // that it starts on the operands its predecessor ended with (cxk_context::lmi_order_forward turns that off)
  unsigned schur_launches = 0;
  // kLmiDense, the side copies of the matrices (UploadLmiDense)
  DevBuf<double> Apad;   // lmi_schur_mfma at a padded order: [A_1 .. A_m | C] per member, zero-padded (LmiMfmaPaddedOrder)
  DevBuf<double> Aleft;  // Hermitian C / H groups on the GEMM assembly: first n / herm_d columns of [A_i | C]
  DevBuf<double> Apk;    // packed lower triangles of the A_i (LmiGroup::Apk), may be empty
  // The large-order work space (MakeLargeWs): the GEMM assembly of kLmiDense, and the step kernels of every `large` or
  // not LDS-resident group of the three routes.
  // ws_main: P and P' during the GEMM assembly, the step temporaries afterwards.  kLmiSparse: C W and X = W C W during
  // assembly, or with the affine term by nonzeros (W C)' in the first half and the values at the positions in the
  // second.  kLmiFactored: the step temporaries.
  DevBuf<double> ws_main;
  DevBuf<double> ws_gf;    // the GEMM assembly's output
  DevBuf<double> ws_part;  // its split partials (`splits` of them); kLmiSparse, kLmiFactored: the slices of the two scalars
  DevBuf<int> ws_piv;      // pivot rows of the step kernels' Pade LU (LmiLargeWs::piv)
  int splits = 1;          // K splits of the GEMM assembly's contraction (AllocGemmAssembly)
  // a `large` group whose Lanczos runs take the chip-wide kernels (kernels_lmi_wide.hip.h, cxk_set_wide_spectrum):
  // their per-constraint work space; empty: lmi_large_spectrum on one workgroup per constraint
  DevBuf<double> ws_wide;
  bool wide_reduce = false;  // ... with lmi_wide_reduce between pass and step (orders from kWideReduceMinOrder on)
  // kLmiSparse: nonzeros matrix-major and position-major instead of the dense A, and the launch split
  struct Sparse {
    int lpp = 1;               // lanes sharing one (i, j) pair sum
    int chunks = 1, emax = 0;  // emax: most nonzeros in one constraint
    bool cdense = false;       // dense affine term: X = W C W instead of pair sums with C
    bool small = false;        // W (and X) of a constraint fit in LDS
    // a Hermitian group over C or H whose sums run over the top block row of every first list (cxk_set_sparse_fold;
    // kernels_lmi_sparse.hip.h, "The folded sums"): the top entries stand first in each list, etop counts them
    bool fold = false;
    DevBuf<int> etop;
    DevBuf<int> eptr, erc, pptr, pvar, pairs;
    DevBuf<double> eval, pval;
  } sp;
  // ... whose dense-route affine term is evaluated from C's nonzeros (cxk_set_sparse_affine; kernels_lmi_sparse.hip.h:
  // lmi_affine_wc / _x / _scalars): every member's C by columns (cptr: n + 1 pointers per member into crc = row | col << 16
  // and cval), the distinct positions of W C W that an entry of some A_i or of C names (pptr: count + 1 pointers
  // into prc = row | col << 16, ascending), and the slot in that list of every entry of the A_i (eslot, beside
  // sp.erc) and of C (cslot, beside crc).
  struct SparseAffine {
    bool on = false;
    int pmax = 0;  // most positions in one member
    DevBuf<int> cptr, crc, cslot, pptr, prc, eslot;
    DevBuf<double> cval;
  } sa;
  // kLmiFactored (cxk_add_lmi_factored): the kernels of kernels_lmi_factored.hip.h in front of the large-order route's
  // (`large` is set: HBM-resident W, ws_main's step temporaries, ws_piv).  Every member's F, sigma, column pointers and
  // column -> variable map; Z, Y, Fs and P in ws (MakeLmiFactored lays it out).  No dense A.
  struct Factors {
    bool rank_one = false;
    int R = 0;
    DevBuf<double> F, sigma, ws;
    DevBuf<int> ptr, var;
  } f;
};

// What every route has.  (Group itself keeps the visibility it always had; the move that std::vector<Group> now makes
// when it grows is new, and stays out of the dynamic symbols.)
struct Group {
  Group() = default;
  CXK_LOCAL Group(Group&&) noexcept = default;
  int type = 0, n = 0, m = 0;
  int herm_d = 0;
  // the set of kernels every member runs on (cone_route.h: Choose)
  ConeRoute route = ConeRoute::kStatic;
  std::vector<int> ids;
  DevBuf<int> dids;
  DevBuf<double> A, C, W, T1;
  LinearState lin;
  SocState soc;
  QuadState quad;
  LmiState lmi;
};
static_assert(!std::is_copy_constructible<Group>::value, "a Group owns its device buffers");
static_assert(std::is_nothrow_move_constructible<Group>::value, "std::vector<Group> moves its groups when it grows");

}  // namespace cxk_host
