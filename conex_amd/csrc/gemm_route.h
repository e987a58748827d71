// Which kernel of gemm_mfma.hip a product runs on and how wide its grid is, as ONE pure function of the call's plain
// fields.  Plain C++17: no HIP, no I/O, no allocation (tests/test_gemm_route.py compiles it alone and walks every
// clause at its edge).  LaunchGemm reads CXK_GEMM_GENERAL, CXK_GEMM_TILE and the CU count, asks ChooseGemm, and
// switches on the route with a case for every enumerator.
#pragma once
#include <cstdint>

namespace cxk_host {

enum class GemmRoute {
  kGeneral,     // gemm_f64_mfma: register-staged, predicated loads (any alignment, odd sizes)
  kDma16,       // gemm_f64_dma<BK = 16>: 64 x 64 tiles, LDS-DMA, four workgroups per CU
  kDma32,       // gemm_f64_dma<BK = 32>: 64 x 64 tiles, two workgroups per CU (long K)
  kDma128x128,  // gemm_f64_dma128<NJ = 4>
  kDma128x64    // gemm_f64_dma128<NJ = 2>
};

constexpr int kGemmRouteBK = 16;  // K granularity of a split (kGemmBK, kernels_gemm.hip.h)

// The fields of a call that the choice reads (GemmArgs, kernels_gemm.hip.h, with pointers as integers).
struct GemmShape {
  int M = 0, N = 0, K = 0;
  int64_t lda = 0, ldb = 0, ldc = 0;
  int64_t sA1 = 0, sA2 = 0, sB1 = 0, sB2 = 0;
  uint64_t a_addr = 0, b_addr = 0;
  bool ta = false, tb = false;
  bool accumulate = false;  // beta != 0
  bool lower_only = false;
  int splits = 1;
  bool has_ct = false;  // a transposed copy-out is asked for (no clause reads it today: every kernel writes one)
  int batch = 1;
};

// What the process is set to: the CU count of the device, CXK_GEMM_TILE (0 = unset) and CXK_GEMM_GENERAL.
struct GemmModes {
  int cus = 256;
  int forced_tile = 0;  // 64 | 128 | 12864
  bool force_general = false;
};

struct GemmLaunch {
  GemmRoute route;
  unsigned grid_x;  // tiles of one matrix and one split (gridDim.y = max(splits, 1), gridDim.z = batch)
};

// The DMA kernels fetch 16-byte chunks (two doubles): every chunk must be aligned and inside its matrix.
// m-major operands: even leading dimension (a pair of rows of one column).  k-major operands: even leading
// dimension and even K (a pair of k of one row).
//
// The two 2^31 clauses bound DmaLane::off[] (gemm_mfma.hip, MakeDmaLane), the byte offset of a lane's chunk from the
// origin of its 64-row image at the start of a stage, kept in 32 bits:
//   k-major image: off = (rc ld + k) 8 with rc <= 63, k <= BK - 2 <= 30        < 64 ld 8      (ld >= K >= 2)
//   m-major image: off = (k ld + rc) 8 with k <= BK - 1 <= 31, rc <= 62; an offset is USED only while k < K (the
//                  others fetch the zero page), so a used off <= ((min(K, 32) - 1) ld + 62) 8 < K ld 8 as soon as
//                  ld >= 63, and is below 2^31 by far when ld < 63.
// The stage advance (a_step, b_step) and the tile origins (a0, b0) are 64-bit.
inline bool GemmDmaEligible(const GemmShape& s, const GemmModes& m) {
  if (m.force_general) return false;  // comparison runs
  if (s.M < 2 || s.N < 2 || s.K < 2) return false;
  if ((s.lda & 1) || (s.ldb & 1) || (s.sA1 & 1) || (s.sA2 & 1) || (s.sB1 & 1) || (s.sB2 & 1)) return false;
  if ((s.a_addr & 15) || (s.b_addr & 15)) return false;
  if ((s.ta || !s.tb) && (s.K & 1)) return false;
  if ((s.ta ? 64 * s.lda : (int64_t)s.K * s.lda) * 8 >= (1ll << 31)) return false;
  if ((!s.tb ? 64 * s.ldb : (int64_t)s.K * s.ldb) * 8 >= (1ll << 31)) return false;
  return true;
}

// Which tile a DMA-eligible product takes: 0 = the 64 x 64 kernel, 4 = 128 x 128, 2 = 128 x 64.  The big tiles need
// enough workgroups to fill the chip (two per CU are resident) and more than one 64-row tile of rows to be worth it;
// forced_tile = 64 | 128 | 12864 forces the choice (comparison runs).
inline int GemmChooseTile(const GemmShape& s, const GemmModes& m) {
  if (m.forced_tile == 64) return 0;
  if (s.M <= 32 && s.N <= 32) return 0;  // (the Gram products share one quadrant: gemm_f64_dma)
  if (s.accumulate && s.splits <= 1) return 0;  // (accumulating calls: the 64 x 64 kernel fetches the old values before its K loop)
  if (m.forced_tile == 128) return 4;
  if (m.forced_tile == 12864) return 2;
  if (s.M <= 64) return 0;  // (implied by clean(M, 128) below: a side of at most 64 has remainder <= 112; kept as moved)
  const int cus = m.cus > 0 ? m.cus : 256;
  // (a ragged last tile of 1 .. 6 sub-tiles a side leaves the four workgroups of an order-200 matrix with
  // shares of 16 / 12 / 12 / 9 MFMA tiles: measured 0.377 against 0.391 of the MFMA peak for the 64 x 64 tiles)
  auto clean = [](int n, int t) { return n % t == 0 || n % t > t - 16; };
  if (!clean(s.M, 128)) return 0;
  const int64_t reps = (int64_t)(s.splits > 1 ? s.splits : 1) * s.batch * ((s.M + 127) / 128);
  // (N > 64 is implied by clean(N, 128) in the same way)
  if (s.N > 64 && clean(s.N, 128) && reps * ((s.N + 127) / 128) >= cus) return 4;
  if (clean(s.N, 64) && reps * ((s.N + 63) / 64) >= 2 * cus) return 2;
  return 0;
}

inline GemmLaunch ChooseGemm(const GemmShape& s, const GemmModes& m) {
  const unsigned tiles_m = (unsigned)((s.M + 63) / 64), tiles_n = (unsigned)((s.N + 63) / 64);
  if (!GemmDmaEligible(s, m)) return {GemmRoute::kGeneral, tiles_m * tiles_n};
  if (const int nj = GemmChooseTile(s, m)) {
    const unsigned tm = (unsigned)((s.M + 127) / 128);
    if (nj == 4) return {GemmRoute::kDma128x128, tm * (unsigned)((s.N + 127) / 128)};
    return {GemmRoute::kDma128x64, tm * tiles_n};
  }
  // a square lower-only call launches the tiles on and below the diagonal only (64 x 64 DMA kernels)
  const unsigned grid_x = (s.lower_only && s.M == s.N) ? tiles_m * (tiles_m + 1) / 2 : tiles_m * tiles_n;
  // k-values per stage: BK = 32 for long K, BK = 16 (more workgroups in flight per CU) otherwise
  const int splits = s.splits > 1 ? s.splits : 1;
  const int ksteps = (s.K + kGemmRouteBK - 1) / kGemmRouteBK;
  const int per_split = (ksteps + splits - 1) / splits * kGemmRouteBK;
  return {per_split >= 512 ? GemmRoute::kDma32 : GemmRoute::kDma16, grid_x};
}

}  // namespace cxk_host
