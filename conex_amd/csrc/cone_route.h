// Which set of kernels a constraint runs on, as ONE pure function of its shape and the modes in force at
// cxk_finalize; and, for a group of matrix inequalities, how its Schur complement is assembled.  Plain C++17: no
// HIP, no I/O, no allocation (tests/test_cone_route.py compiles it alone and walks the modes and the shape edges).
// Also here, because admission and the launch sites must read ONE definition: the dynamic-LDS need of every
// LDS-resident kernel, and the thresholds of the automatic modes.
//
// GroupConstraints (kkt_cone_launch.hip) measures a constraint, asks Choose, and raises the refusal or stores the
// route; every stage of the cxk_* path then switches on Group::route with a case for every enumerator, and each case
// calls the unit that owns the route's kernels (cone_units.h: cone_linear / _soc / _quad / _lmi .hip).
#pragma once
#include <climits>
#include <cstddef>
#include <cstdint>

#include "../../include/conex_kkt_hip.h"  // the CXK_* constraint types (a C header)

namespace cxk_host {

constexpr size_t kLdsLimit = 160 * 1024 - 512;

// One enumerator per set of kernels.
enum class ConeRoute {
  kLinearLds,     // one workgroup per block (kernels_linear.hip.h)
  kLinearTiled,   // kernels_linear_tiled.hip.h
  kLinearSparse,  // from the nonzeros (kernels_linear_sparse.hip.h)
  kSocLds,        // one wavefront per cone, its image in LDS (kernels_soc.hip.h)
  kSocStreamed,   // held in HBM (kernels_soc_stream.hip.h)
  kSocSparse,     // from the nonzeros (kernels_soc_sparse.hip.h)
  kQuadLds,       // one workgroup per cone (kernels_quad.hip.h)
  kQuadStreamed,  // held in HBM (kernels_quad_stream.hip.h)
  kLmiDense,      // dense matrices: the LmiKernel choosers name the instance of each stage
  kLmiSparse,     // from the nonzeros (kernels_lmi_sparse.hip.h)
  kLmiFactored,   // from the factors, in front of the large-order kernels (kernels_lmi_factored.hip.h)
  kStatic,        // constant Schur block
  kOct            // kernels_oct.hip.h
};

// How a group of matrix inequalities assembles its Schur complement.
enum class LmiAssembly {
  kGeneric,  // the route's own kernels (lmi_schur_generic, the sparse sums, the factored products)
  kMfma,     // lmi_schur_mfma (lmi_fused_mfma.hip)
  kGemm      // the batched MFMA GEMM pipeline (kernels_lmi_large.hip.h)
};

// The widest linear block the LDS route can run: linear_line_search is launched with 16 m bytes of dynamic LDS
// and has the default limit of 64 KB (linear_prepare's 8 m bytes reach it at 8192).
constexpr int kLinearLdsMaxVars = 4096;
// Automatic mode sends a linear block of rows x m to the tiled route from rows m^2 >= this on.  Measured
// (tools/linear_tiled_speed.py against the build before the tiled route): twice the smallest
// rows m^2 among the measured shapes from which assembly, PrepareStep and the eigenvalue query are each faster on
// the tiled route at that shape and at every larger one, 2000 x 64 (at 256 x 32 the assembly is five times faster
// but the two-launch PrepareStep and query cost 2 us more); twice, because the numbers are one box's on one day.
constexpr long long kTiledLinearMinWork = 2ll * 2000 * 64 * 64;  // 16 384 000

// Automatic mode (cxk_set_sparse_linear(ctx, -1)) sends a linear block to the sparse route when
// R sum_r nnz_r^2 <= rows m^2: the sparse assembly forms about sum_r nnz_r^2 products one fma at a time, the dense
// routes rows m^2 on the matrix pipe.  Measured (tools/linear_sparse_speed.py against the build before the sparse
// route on its own choice): R is twice the smallest rows m^2 / sum_r nnz_r^2 among the measured
// shapes at which assembly, PrepareStep and the eigenvalue query are each faster on the sparse route, 3.9 at the
// half-full 2000 x 64; twice, because the numbers are one box's on one day.  A fully dense block (ratio 1) never moves.
// CXK_SPARSE_LINEAR_MIN_RATIO moves R for comparison runs.  Two more conditions, both from shapes that lost:
//  - a column's rows are one wavefront's dependent chain, 0.33 us per row (100 000 x 50 with one full column: 32.6 ms
//    against 0.38 ms): no column longer than kSparseLinearMaxColumn, twice the longest measured to win (about 1050);
//  - a thousand 20 x 10 blocks with 3 nonzeros per row are 20 % slower at every stage than on the LDS route's one
//    launch per stage: nothing below the rows m^2 of the smallest measured shape that won, 2000 x 64, moves.
constexpr double kSparseLinearMinRatio = 7.8;
constexpr int kSparseLinearMaxColumn = 2048;
constexpr long long kSparseLinearMinWork = 2000ll * 64 * 64;  // 8 192 000
inline bool LinearSparsePays(double rows, double m, double sum_nnz_sq, int longest_column, double ratio) {
  return ratio * sum_nnz_sq <= rows * m * m && rows * m * m >= (double)kSparseLinearMinWork &&
         longest_column <= kSparseLinearMaxColumn;
}

// Automatic mode (cxk_set_sparse_soc(ctx, -1)) sends a second-order cone of dimension len = n + 1 over m variables to
// the sparse route when it can run nowhere else (added by cxk_add_soc_csr, or len m beyond the int range), or when
// R nnz <= len m and len m^2 >= kSparseSocMinWork: the sparse assembly reads the nnz nonzeros and moves the m x m
// square twice, the dense routes stream len m entries (and the streamed one multiplies len m^2).  Measured
// (tools/soc_sparse_speed.py --sweep against the streamed route): each constant is twice the smallest
// value among the swept shapes at which assembly + query + PrepareStep + TakeStep are faster on the sparse route;
// twice, because the numbers are one box's on one day.  The smallest winning len m / nnz is 2.02 (2048 x 64 half full:
// 87.8 us against 129.7 us; the assembly gains 4.3x, the one-thread-per-row slack loses 0.63x); a fully dense 401 x 61
// loses (87.6 us against 82.7 us) and never moves.  The smallest swept shape, 401 x 61 (len m^2 = 1 492 121), wins at
// 3 nonzeros per row (51.4 us against 79.7 us); nothing smaller was measured, so nothing smaller moves.
// CXK_SPARSE_SOC_MIN_RATIO moves R for comparison runs.  No default anywhere asks for this mode.
constexpr double kSparseSocMinRatio = 4.04;
constexpr long long kSparseSocMinWork = 2ll * 401 * 61 * 61;  // 2 984 242
inline bool SocSparsePays(double len, double m, double nnz, double ratio) {
  return ratio * nnz <= len * m && len * m * m >= (double)kSparseSocMinWork;
}

// Automatic mode (cxk_set_streamed_quadratic(ctx, -1)) sends a quadratic cone to the streamed route from this many
// doubles streamed per pass, (Q ? n n : 0) + (n + 1) m, on.  Measured (tools/quad_stream_speed.py):
// the smallest shape of the sweep, n = 32 with Q over m = 8 (32 * 32 + 33 * 8), where assembly + PrepareStep +
// TakeStep already take 48 us on the streamed route against 333 us on the LDS route; every larger swept shape gains
// more.  Nothing smaller was measured, so nothing smaller moves (the cones of a handful of doubles stay where they are).
constexpr long long kQuadStreamMinWork = 32 * 32 + 33 * 8;  // 1288

// A quadratic cone whose Q = S + F diag(sigma) F' is given by its parts (cxk_add_quadratic_structured,
// kernels_quad_structured.hip.h).  How many lanes work on one row of S, from the mean nonzeros per row of the group: one
// lane is a chain as long as the row, 64 lanes leave most of a wavefront idle on a short row.  Measured
// (tools/quad_structured_speed.py --lanes, DESIGN.md 4.10.2: one cone, n = 16384, m = 8, rank 8, band matrices of 3, 9,
// 27, 81 and 243 nonzeros per row, assembly + PrepareStep + TakeStep in us under 1 / 8 / 64 lanes): 255 / 268 / 363,
// 256 / 271 / 368, 284 / 288 / 371, 363 / 330 / 414, 784 / 559 / 615.  One lane is the fastest up to 27 per row (a tie
// with eight there), eight lanes from 81 on; 64 lanes won at no swept width.  So: one lane up to the largest width at
// which it did not lose, eight up to the largest width measured; beyond 243 per row NOTHING was measured and the step to
// 64 lanes there is a guess (the trend, 1.26 times the 8-lane time at 81 and 1.10 times at 243, is all that speaks for it).
// One box, one day.  CXK_QUAD_CSR_LANES = 1 | 8 | 64 overrides the rule.
constexpr double kQuadCsrOneLaneMaxMean = 27;
constexpr double kQuadCsrEightLanesMaxMean = 243;
inline int QuadCsrLanes(double nnz, double rows) {
  const double mean = rows > 0 ? nnz / rows : 0;
  return mean <= kQuadCsrOneLaneMaxMean ? 1 : mean <= kQuadCsrEightLanesMaxMean ? 8 : 64;
}
// Row segments of the factor dots F' x of `columns` = cones x rank columns of n rows: enough workgroups to fill the
// chip (as QuadStreamSplits: 512), none shorter than kQuadFactorMinSegment rows (four per thread of a workgroup).
constexpr int kQuadFactorMinSegment = 1024;
inline int QuadFactorSegments(int n, long long columns) {
  const long long cols = columns > 0 ? columns : 1;
  const long long by_len = n / kQuadFactorMinSegment, by_fill = (512 + cols - 1) / cols;
  const long long s = by_len < by_fill ? by_len : by_fill;
  return s < 1 ? 1 : (int)s;
}

// A quadratic cone whose A is held by its nonzeros (cxk_add_quadratic_csr, kernels_quad_sparse.hip.h) forms
// A_gram = A1' Q A1 at cxk_finalize in panels of P columns of A1: the panel and T = Q panel, n x P each per cone, are
// all the work space, whatever m is.  P from a fixed budget of bytes for the two buffers of the whole group, at least
// kQuadGramPanelMinCols (the column tile of quad_struct_sa) and at most kQuadGramPanelMaxCols (a handful of launches
// per 64 columns is amortised; a wider panel of a small cone would only cost memory).  Neither bound was tuned.
constexpr long long kQuadGramPanelBytes = 256ll << 20;
constexpr int kQuadGramPanelMinCols = 4;
constexpr int kQuadGramPanelMaxCols = 64;
inline int QuadGramPanelCols(int n, long long count) {
  const long long per_col = 2 * 8 * (count > 0 ? count : 1) * (n > 0 ? n : 1);
  const long long p = kQuadGramPanelBytes / per_col;
  return p < kQuadGramPanelMinCols ? kQuadGramPanelMinCols : p > kQuadGramPanelMaxCols ? kQuadGramPanelMaxCols : (int)p;
}

// Automatic mode (cxk_set_sparse_affine(ctx, -1)) evaluates the affine term C of a sparse matrix inequality beyond
// the LDS-resident orders from C's nonzeros (kernels_lmi_sparse.hip.h: lmi_affine_wc, lmi_affine_x) when
// R (nnz_c + npos) <= 4 n^2: the two kernels make n nnz_c + n npos multiply-adds (npos: the distinct positions of
// W C W that an entry of some A_i or of C names), the two GEMMs they replace 4 n^3 flops on the matrix pipe.  Measured
// (tools/lmi_entries_speed.py): R is twice the smallest 4 n^2 / (nnz_c + npos) among the measured
// shapes at which the assembly is faster on the new kernels, 30.6 at order 256 with 8 sub-diagonals (42.8 us against
// 54.6 us); every measured shape with a larger ratio wins too (max-cut at 500 / 2000: 143 / 572), every one at 20 and
// below loses (a tenth of C's entries at order 256 / 1024: 58.1 us against 54.2 us, 274 us against 151 us); twice,
// because the numbers are one box's on one day.  CXK_SPARSE_AFFINE_MIN_RATIO moves R for comparison runs.  An affine
// term of at most kSparseAffineMinNnz nonzeros never asks: it rides in the pair sums as list number m.
constexpr double kSparseAffineMinRatio = 61.2;
constexpr int kSparseAffineMinNnz = 64;
inline bool LmiSparseAffinePays(double n, double nnz_c, double npos, double ratio = kSparseAffineMinRatio) {
  return nnz_c > kSparseAffineMinNnz && ratio * (nnz_c + npos) <= 4.0 * n * n;
}
// The packed tables of the sparse-LMI route (erc = row | col << 16, the pair table i | j << 16) go into ints that the
// kernels unpack with `& 0xffff` and a signed `>> 16`: the shifted half must stay below 2^15.  cxk_add_lmi_coo
// refuses a larger order or variable count by this name.
constexpr int kSparseLmiMaxIndex = 32767;

// Dynamic LDS of the LDS-resident kernels: what the launch sites ask for and what Choose admits a constraint by,
// so that an admitted constraint can be launched at every stage.  Every product is taken in size_t.
inline size_t LmiGenericLds(int n) { return sizeof(double) * 4 * (size_t)n * (size_t)n; }
inline size_t LmiPrepareLds(int n, int m) { return sizeof(double) * (3 * (size_t)n * n + 6 * (size_t)n + 2 * ((size_t)n / 2 + 2) + m + 8); }
inline size_t LmiTakeLds(int n) { return sizeof(double) * 5 * (size_t)n * (size_t)n; }
inline size_t SocSchurLds(int n, int m, bool staged) { return sizeof(double) * ((size_t)n + 1) * (staged ? 2 * (size_t)m + 4 : (size_t)m + 2); }
inline size_t SocPrepareLds(int n, int m) { return sizeof(double) * ((size_t)m + 3 * ((size_t)n + 1)); }
inline size_t SocTakeLds(int n) { return sizeof(double) * 4 * ((size_t)n + 1); }
inline size_t QuadSchurLds(int n, int m) { return sizeof(double) * (2 * (size_t)n + (size_t)m + 4); }
inline size_t QuadPrepareLds(int n, int m) { return sizeof(double) * ((size_t)m + 4 * ((size_t)n + 1)); }
inline size_t QuadTakeLds(int n) { return sizeof(double) * 3 * ((size_t)n + 1); }
// the LDS-resident orders of a matrix inequality: beyond them the large-order kernels (Group::lmi.large)
inline bool LmiLdsResident(int n, int m) { return LmiTakeLds(n) <= kLdsLimit && LmiPrepareLds(n, m) <= kLdsLimit; }

// What is known of one constraint when its route is chosen.
struct ConeShape {
  int type = 0, n = 0, m = 0, herm_d = 0;  // CXK_LMI ..., the sizes as cxk_add_* took them
  bool symmetric = true;  // CXK_LMI: every A_i and C equals its transpose
  // added by its nonzeros (no dense matrix; CXK_QUAD: cxk_add_quadratic_csr, `nnz` below is set); CXK_LMI given by
  // factors; CXK_QUAD with an inner-product matrix
  bool csr_only = false, factored = false, has_q = false;
  // the nonzeros of a linear block or a second-order cone, measured only while its sparse mode is not 0
  bool nnz_fits_int = true;  // their count is within the int range
  double nnz = 0;            // their count
  double sum_nnz_sq = 0;     // sum over the rows of the squared count
  int longest_column = 0;
  // CXK_LMI: the predicates that live beside the kernels, already evaluated
  bool mfma_supports = false;  // LmiMfmaSupports(n, m, herm_d)
  bool sparse_pays = false;    // LmiSparsePays(n, m, nonzeros of A, LmiLdsResident(n, m), mfma_supports)
  // CXK_QUAD whose Q = S + F diag(sigma) F' is held by its parts (has_q is set too): the nonzeros of S, the rank
  bool q_structured = false;
  double q_nnz = 0;
  int q_rank = 0;
};

// The modes in force: what the context was told (cxk_set_*), else the environment's word, else the default here
// (GroupConstraints resolves them once), and the thresholds of the automatic ones.
struct RouteModes {
  bool streamed_cones = false;  // CXK_STREAMED_CONES=1: second-order cones beyond LDS are held in HBM (else refused)
  int tiled_linear = -1;        // CXK_TILED_LINEAR: -1 by size, 0 never, 1 every block
  int streamed_quadratic = 0;   // CXK_STREAMED_QUADRATIC: -1 by size, 0 never, 1 every cone
  int sparse_linear = 0;        // CXK_SPARSE_LINEAR: -1 by pattern, 0 never, 1 every block
  int sparse_soc = 0;           // CXK_SPARSE_SOC: -1 by pattern, 0 never, 1 every cone
  int sparse_lmi = -1;          // CXK_SPARSE_LMI: -1 when it pays, 0 never, 1 always (tests)
  long long tiled_linear_min_work = kTiledLinearMinWork;            // CXK_TILED_LINEAR_MIN_WORK (comparison runs)
  long long streamed_quadratic_min_work = kQuadStreamMinWork;       // CXK_STREAMED_QUADRATIC_MIN_WORK (comparison runs)
  double sparse_linear_min_ratio = kSparseLinearMinRatio;           // CXK_SPARSE_LINEAR_MIN_RATIO (comparison runs)
  double sparse_soc_min_ratio = kSparseSocMinRatio;                 // CXK_SPARSE_SOC_MIN_RATIO (comparison runs)
  // CXK_SPARSE_AFFINE: how a sparse LMI group beyond the LDS-resident orders evaluates an affine term of more than 64
  // nonzeros: -1 from C's nonzeros when LmiSparseAffinePays, 0 by the two GEMMs, 1 always from the nonzeros; -2: nobody
  // said, each constraint keeps the default of its entry point (cxk_add_lmi 0, cxk_add_lmi_coo -1).  No route hangs on it.
  int sparse_affine = -2;
  double sparse_affine_min_ratio = kSparseAffineMinRatio;           // CXK_SPARSE_AFFINE_MIN_RATIO (comparison runs)
  // CXK_SPARSE_FOLD: whether a sparse Hermitian LMI group over C or H sums over the top block row of its real
  // representations (kernels_lmi_sparse.hip.h, "The folded sums"): 0 never, 1 always; -2: nobody said, each constraint
  // keeps the default of its entry point (cxk_add_hermitian 0, cxk_add_hermitian_coo 1).  No route hangs on it.
  int sparse_fold = -2;
};

// The route, or why there is none (`refusal` is the message cxk_finalize fails with; null with a route).
struct RouteChoice {
  ConeRoute route;
  const char* refusal;
};

namespace route_detail {
constexpr RouteChoice Take(ConeRoute r) { return RouteChoice{r, nullptr}; }
constexpr RouteChoice Refuse(const char* why) { return RouteChoice{ConeRoute::kStatic, why}; }
// (rows x max(m, 1) entries indexed with ints by the kernels and by the GEMM)
inline bool EntriesFitInt(int64_t rows, int m) { return rows * (m > 1 ? m : 1) <= INT_MAX - 1024; }
inline bool SquareFitsInt(int m) { return (int64_t)m * m <= INT_MAX; }

inline RouteChoice ChooseLinear(const ConeShape& s, const RouteModes& md) {
  if (s.csr_only && md.sparse_linear == 0)
    return Refuse("a linear block added by cxk_add_linear_csr has no dense matrix and can only take the sparse route "
                  "(cxk_set_sparse_linear / CXK_SPARSE_LINEAR, which is 0)");
  if (!s.nnz_fits_int && md.sparse_linear == 1)  // (the pointers are ints)
    return Refuse("a sparse linear block with more than 2^31 nonzeros is not supported");
  bool sparse = s.csr_only || md.sparse_linear == 1;
  // automatic mode yields to an explicit tiled mode, which asks for the dense kernels
  if (md.sparse_linear == -1 && !s.csr_only && md.tiled_linear < 0 && s.nnz_fits_int)
    sparse = LinearSparsePays(s.n, s.m, s.sum_nnz_sq, s.longest_column, md.sparse_linear_min_ratio);
  if (sparse) {
    if (!SquareFitsInt(s.m))
      return Refuse("a sparse linear block whose variables x variables Schur block exceeds the int range is not supported");
    return Take(ConeRoute::kLinearSparse);
  }
  const bool tiled = md.tiled_linear >= 0 ? md.tiled_linear != 0
                                          : s.m > kLinearLdsMaxVars ||
                                                (double)s.n * s.m * s.m >= (double)md.tiled_linear_min_work;
  if (tiled) {
    // what remains is the int indexing of the kernels and of the GEMM
    if (!EntriesFitInt(s.n, s.m))
      return Refuse("a tiled linear block whose rows x variables entries exceed the int range is not supported");
    if (!SquareFitsInt(s.m))
      return Refuse("a tiled linear block whose variables x variables Schur block exceeds the int range is not supported");
    return Take(ConeRoute::kLinearTiled);
  }
  // linear_line_search keeps two vectors of m doubles in 64 KB of dynamic LDS
  if (s.m > kLinearLdsMaxVars)
    return Refuse("a linear block over more than 4096 variables does not fit the LDS route's kernels: it needs the tiled "
                  "route (cxk_set_tiled_linear / CXK_TILED_LINEAR, which was set to 0)");
  return Take(ConeRoute::kLinearLds);
}

inline RouteChoice ChooseSoc(const ConeShape& s, const RouteModes& md) {
  if (s.csr_only && md.sparse_soc == 0)
    return Refuse("a second-order cone added by cxk_add_soc_csr has no dense matrix and can only take the sparse route "
                  "(cxk_set_sparse_soc / CXK_SPARSE_SOC, which is 0)");
  if (!s.nnz_fits_int && md.sparse_soc == 1)  // (the pointers are ints)
    return Refuse("a sparse second-order cone with more than 2^31 nonzeros is not supported");
  // (a dense route indexes the (n + 1) x m entries with ints)
  const bool dense_ok = EntriesFitInt((int64_t)s.n + 1, s.m);
  bool sparse = s.csr_only || md.sparse_soc == 1;
  if (md.sparse_soc == -1 && !s.csr_only && s.nnz_fits_int)
    sparse = !dense_ok || SocSparsePays((double)s.n + 1, s.m, s.nnz, md.sparse_soc_min_ratio);
  if (sparse) {
    // held as nonzeros: no LDS room, no streamed switch; what remains is the int indexing of the m x m squares H and G
    if (!SquareFitsInt(s.m))
      return Refuse("a sparse second-order cone whose variables x variables Schur block exceeds the int range is not supported");
    return Take(ConeRoute::kSocSparse);
  }
  const bool steps_fit = SocTakeLds(s.n) <= kLdsLimit && SocPrepareLds(s.n, s.m) <= kLdsLimit;
  const bool image_fits = SocSchurLds(s.n, s.m, false) <= kLdsLimit;
  if (md.streamed_cones && !(image_fits && steps_fit)) {
    // held in HBM: what remains is the int indexing of the kernels and of the GEMM
    if (!dense_ok)
      return Refuse("a streamed second-order cone whose (dimension + 1) x variables entries exceed the int range is not supported");
    if (!SquareFitsInt(s.m))
      return Refuse("a streamed second-order cone whose variables x variables Schur block exceeds the int range is not supported");
    return Take(ConeRoute::kSocStreamed);
  }
  // soc_schur keeps a cone's (n + 1) x (m + 2) image in LDS (CONEX_NewLorentzConeConstraint makes a
  // cone's matrix as wide as its largest variable index: thousands of columns are possible there)
  if (!image_fits)
    return Refuse("a second-order cone whose (dimension + 1) x (variables + 2) image exceeds LDS (160 KB) is not supported");
  // soc_take_step keeps four vectors of the cone in LDS, soc_prepare three and y: with one variable
  // they, not the image above, are what has to fit
  if (!steps_fit)
    return Refuse("a second-order cone whose step kernels need more than the 163 328 B of LDS (four vectors of dimension + 1) is "
                  "not supported");
  return Take(ConeRoute::kSocLds);
}

inline RouteChoice ChooseQuad(const ConeShape& s, const RouteModes& md) {
  // held by the parts of Q: no LDS form, whatever the switch says; n x n is never formed, so only the nonzeros of S
  // (ints on the device, per group: UploadQuadStructured) and the two demands of every streamed cone remain
  if (s.q_structured) {
    if (!s.csr_only && !EntriesFitInt((int64_t)s.n + 1, s.m))
      return Refuse("a streamed quadratic cone whose (dimension + 1) x variables entries exceed the int range is not supported");
    if (s.csr_only && s.nnz > (double)INT_MAX)
      return Refuse("a quadratic cone added by cxk_add_quadratic_csr with more than 2^31 nonzeros is not supported");
    if (!SquareFitsInt(s.m))
      return Refuse("a streamed quadratic cone whose variables x variables Schur block exceeds the int range is not supported");
    if (s.q_nnz > (double)INT_MAX)
      return Refuse("a structured quadratic cone whose sparse part has more than 2^31 nonzeros is not supported");
    return Take(ConeRoute::kQuadStreamed);
  }
  // held by the nonzeros of A (cxk_add_quadratic_csr; ConeShape::nnz counts them): no LDS form either, and nothing
  // of (n + 1) x m exists to be indexed; the Schur block, a dense Q and the int pointers of the nonzeros remain
  if (s.csr_only) {
    if (!SquareFitsInt(s.m))
      return Refuse("a streamed quadratic cone whose variables x variables Schur block exceeds the int range is not supported");
    if (s.has_q && !SquareFitsInt(s.n))
      return Refuse("a streamed quadratic cone whose inner-product matrix has more than 2^31 entries is not supported");
    if (s.nnz > (double)INT_MAX)
      return Refuse("a quadratic cone added by cxk_add_quadratic_csr with more than 2^31 nonzeros is not supported");
    return Take(ConeRoute::kQuadStreamed);
  }
  // quad_prepare keeps y and four vectors of the cone in LDS; quad_schur and quad_take_step need less
  const bool fits = QuadPrepareLds(s.n, s.m) <= kLdsLimit && QuadSchurLds(s.n, s.m) <= kLdsLimit && QuadTakeLds(s.n) <= kLdsLimit;
  const double work = (s.has_q ? (double)s.n * s.n : 0.0) + ((double)s.n + 1) * s.m;  // doubles streamed per pass
  const bool streamed = md.streamed_quadratic >= 0 ? md.streamed_quadratic != 0
                                                   : !fits || work >= (double)md.streamed_quadratic_min_work;
  if (streamed) {
    // held in HBM: what remains is the int indexing of the kernels and of the GEMM
    if (!EntriesFitInt((int64_t)s.n + 1, s.m))
      return Refuse("a streamed quadratic cone whose (dimension + 1) x variables entries exceed the int range is not supported");
    if (!SquareFitsInt(s.m))
      return Refuse("a streamed quadratic cone whose variables x variables Schur block exceeds the int range is not supported");
    if (s.has_q && !SquareFitsInt(s.n))
      return Refuse("a streamed quadratic cone whose inner-product matrix has more than 2^31 entries is not supported");
    return Take(ConeRoute::kQuadStreamed);
  }
  if (!fits)
    return Refuse("a quadratic cone whose step kernels need more than the 163 328 B of LDS (variables + four vectors of "
                  "dimension + 1) is not supported");
  return Take(ConeRoute::kQuadLds);
}

inline RouteChoice ChooseLmi(const ConeShape& s, const RouteModes& md) {
  // held by its factors in front of the large-order route (cxk_finalize has checked the order and the int indexing
  // of the kernels)
  if (s.factored) return Take(ConeRoute::kLmiFactored);
  // held by its nonzeros (symmetric by construction, order and variables within kSparseLmiMaxIndex: cxk_add_lmi_coo)
  // (a Hermitian one, herm_d set: cxk_add_hermitian_coo)
  if (s.csr_only) {
    if (md.sparse_lmi == 0)
      return Refuse(s.herm_d > 0
                        ? "a matrix inequality added by cxk_add_hermitian_coo has no dense matrices and can only take the sparse "
                          "route (CXK_SPARSE_LMI, which is 0)"
                        : "a matrix inequality added by cxk_add_lmi_coo has no dense matrices and can only take the sparse route "
                          "(CXK_SPARSE_LMI, which is 0)");
    return Take(ConeRoute::kLmiSparse);
  }
  // The reference accepts non-symmetric matrices and evaluates <W A_i W, A_j> as written; only the literal LDS
  // kernels do the same.
  if (!s.symmetric && !LmiLdsResident(s.n, s.m))
    return Refuse("non-symmetric LMI data beyond the LDS-resident orders is not supported: "
                  "the large-order kernels use tr(W A_i W A_j) = tr(P_i P_j), which needs A_i = A_i^T");
  // sparse evaluation when it pays (CXK_SPARSE_LMI=0 / 1 forces never / always: tests); its entries are packed
  // row | col << 16
  const bool sparse = (md.sparse_lmi >= 0 ? md.sparse_lmi != 0 : s.sparse_pays) && s.n <= 65535 && s.symmetric;
  return Take(sparse ? ConeRoute::kLmiSparse : ConeRoute::kLmiDense);
}
}  // namespace route_detail

inline RouteChoice Choose(const ConeShape& shape, const RouteModes& modes) {
  switch (shape.type) {
    case CXK_LMI: return route_detail::ChooseLmi(shape, modes);
    case CXK_LINEAR: return route_detail::ChooseLinear(shape, modes);
    case CXK_SOC: return route_detail::ChooseSoc(shape, modes);
    case CXK_QUAD: return route_detail::ChooseQuad(shape, modes);
    case CXK_OCT: return route_detail::Take(ConeRoute::kOct);
    default: return route_detail::Take(ConeRoute::kStatic);
  }
}

// The assembly of a group of `count` matrix inequalities on `route`, and whether the group runs on the large-order
// kernels (HBM-resident matrices).  Shapes past the register kernels' instances assemble through the batched GEMM
// (measured 1.5 - 3.3x faster than lmi_schur_generic at 1000 constraints: orders 25 up, and smaller orders with
// more variables than lmi_schur_mfma's LDS images hold, e.g. order 22, m = 20 285 -> 133 us, order 10, m = 60
// 496 -> 148 us; CXK_GEMM_MIN_N moves the threshold for comparison runs), while its work space stays within 8 GB.
struct LmiAssemblyChoice {
  bool large;
  LmiAssembly assembly;
};
inline LmiAssemblyChoice ChooseLmiAssembly(ConeRoute route, int n, int m, size_t count, bool literal, bool mfma_supports,
                                           bool schur_generic, int gemm_min_n) {
  // held by its factors in front of the large-order route, whatever its order
  if (route == ConeRoute::kLmiFactored) return {true, LmiAssembly::kGeneric};
  const bool large = !LmiLdsResident(n, m);
  if (route != ConeRoute::kLmiDense || literal) return {large, LmiAssembly::kGeneric};
  if (large) return {true, LmiAssembly::kGemm};
  if (!schur_generic && mfma_supports) return {false, LmiAssembly::kMfma};
  const bool gemm = n >= gemm_min_n &&
                    count * 2 * ((size_t)m + 1) * (size_t)n * (size_t)n * sizeof(double) <= ((size_t)8 << 30);
  return {false, gemm ? LmiAssembly::kGemm : LmiAssembly::kGeneric};
}

}  // namespace cxk_host
