// The dense elimination core: row-per-lane right-looking Cholesky steps in registers, column
// updates as DPP fmas.  Device functions and templates only; knows nothing of the tree (no
// FactorPlan, no SnRec).  Used by the supernode building blocks (tree_supernode.hip.h:
// FactorSupernodeRows describes the register layout), the dense top (kernels_kkt_top.hip.h),
// the blocked big-supernode kernels (big_chol.hip, big_panel_solve.hip.h, kernels_kkt_big.hip.h),
// the whole-tree launch (tree_fused.hip) and kernels_lmi_rows.hip.h (DppOperandFence).
#pragma once
#include "device_utils.h"

namespace cxk {

// L_jj = sqrt(d) and 1/L_jj from one v_rsq_f64 refined by two Goldschmidt iterations.
__device__ __forceinline__ void SqrtAndInverse(double d, double& root, double& inv) {
  const double r0 = __builtin_amdgcn_rsq(d);
  double g = d * r0, h = 0.5 * r0;
  double e = fma(-h, g, 0.5);
  g = fma(g, e, g);
  h = fma(h, e, h);
  e = fma(-h, g, 0.5);
  g = fma(g, e, g);
  h = fma(h, e, h);
  const double res = fma(-g, g, d);  // final correction: root is within 1 ulp of sqrt(d)
  root = fma(res, h, g);
  inv = h + h;
}

// a[c] += w[lane (c - BASE) of the own 16-lane DPP row] * v   for c in [C0, C1).
template <int LEN, int C0, int C1, int BASE>
struct DppColumns {
  static __device__ __forceinline__ void run(double (&a)[LEN], double w, double v) {
    if constexpr (C0 < C1) {
      asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
          : "+v"(a[C0])
          : "v"(w), "v"(v), "n"(C0 - BASE));
      DppColumns<LEN, C0 + 1, C1, BASE>::run(a, w, v);
    }
  }
};

// The compiler cannot see that the asm above is a DPP instruction, so the hazard "VALU writes a
// VGPR, a DPP instruction reads it within 2 wait states" is covered by hand: operands pass
// through this fence (s_nop 1) after their last write and before any DPP use.
__device__ __forceinline__ void DppOperandFence(double& x, double& y, double& z) {
  asm("s_nop 1" : "+v"(x), "+v"(y), "+v"(z));
}

// DPP rows 0 and 2 of v copied over rows 1 and 3 (v_permlane16_swap, gfx950).
__device__ __forceinline__ double EvenRowsToOddRows(double v) {
  typedef unsigned u2 __attribute__((ext_vector_type(2)));
  const unsigned lo = __double2loint(v), hi = __double2hiint(v);
  const u2 a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const u2 b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  return __hiloint2double(b.x, a.x);
}

// Elimination steps J .. NSMAX-1 of FactorSupernodeRows (compile-time recursion: every register
// index, lane select and DPP control is an immediate).
// Step J receives sqrt(d_J) and 1/sqrt(d_J) from step J-1, which starts that dependent chain
// (readlane, v_rsq_f64, two Goldschmidt steps: ~130 cycles on a lone wavefront) as soon as column J
// has taken its own update, so that the chain overlaps the remaining column updates of step J-1
// instead of following them.  Same operations on the same values: results are unchanged.
// NRHS right-hand side columns a[RB ..] (1; 3 in the whole-tree launch with three right-hand sides).
// CHECK = false: no test of the pivots (two instructions per pivot on a lone wavefront's critical path): a pivot
// that is not positive leaves NaNs in its column and in everything eliminated behind it, and the caller looks
// for them in what it produces at its end (tree_fused: the solution entries).
template <int NSMAX, int SMAX, int J, int NRHS = 1, bool CHECK = true>
struct ElimSteps {
  static constexpr int LEN = NSMAX + SMAX + NRHS, RB = NSMAX + SMAX;
  // ns = columns of the supernode (wave-uniform): the padding pivots ns .. NSMAX-1 are identity
  // steps (unit diagonal, zero column) and are skipped.
  static __device__ __forceinline__ void run(double (&a)[LEN], int lane, bool& bad, int ns) {
    if constexpr (J == 0 && NSMAX > 0) {
      const double d = ReadLane(a[0], 0);
      if constexpr (CHECK) bad |= !(d > 0.0);
      double root, inv;
      SqrtAndInverse(d, root, inv);
      step(a, lane, bad, root, inv, ns);
    }
  }
  static __device__ __forceinline__ void step(double (&a)[LEN], int lane, bool& bad, double root, double inv, int ns) {
    if constexpr (J < NSMAX) {
      if (J >= ns) return;
      a[J] = (lane == J) ? root : a[J] * inv;
      double root1 = 1.0, inv1 = 1.0;
      auto next_pivot = [&]() {  // column J+1 is final for step J+1 once it has taken column J's term
        if constexpr (J + 1 < NSMAX) {
          const double d1 = ReadLane(a[J + 1], J + 1);
          if constexpr (CHECK) bad |= !(d1 > 0.0);
          SqrtAndInverse(d1, root1, inv1);
        }
      };
      if constexpr (NSMAX + SMAX <= 16) {
        // the whole panel (supernode rows + separator rows) sits in ONE 16-lane DPP row:
        // row_newbcast:c delivers L[c][J] (c < NSMAX) and L[sep c - NSMAX][J] directly
        double naj = -a[J];
        double dummy = 0.0;
        DppOperandFence(dummy, naj, a[J]);
        DppColumns<LEN, J + 1, (J + 2 < NSMAX + SMAX ? J + 2 : NSMAX + SMAX), 0>::run(a, a[J], naj);
        next_pivot();
        DppColumns<LEN, J + 2, NSMAX + SMAX, 0>::run(a, a[J], naj);
      } else if constexpr (NSMAX + SMAX <= 32 && NSMAX != 16) {
        // the panel (supernode rows, then separator rows at lanes NSMAX..) fills DPP rows 0 and 1.
        // Row 0 mirrored into row 1 serves the columns whose owner lane is < 16, row 1 mirrored
        // into row 0 the columns whose owner lane is >= 16.
        const RowPair xp = Swap16(a[J]);
        double x0 = xp.a, x1 = xp.b;
        double naj = -a[J];
        DppOperandFence(x0, x1, naj);
        constexpr int kEnd = NSMAX + SMAX;
        // column J + 1 first, then the chain of the next pivot, then the rest
        constexpr int n1 = (J + 2 < kEnd) ? J + 2 : kEnd;
        if constexpr (J + 1 < 16)
          DppColumns<LEN, J + 1, (n1 < 16 ? n1 : 16), 0>::run(a, x0, naj);
        else
          DppColumns<LEN, J + 1, n1, 16>::run(a, x1, naj);
        next_pivot();
        constexpr int kLo0 = (J + 2 < 16) ? J + 2 : 16, kLo1 = (kEnd < 16) ? kEnd : 16;
        constexpr int kHi0 = (J + 2 > 16) ? J + 2 : 16;
        DppColumns<LEN, kLo0, kLo1, 0>::run(a, x0, naj);
        DppColumns<LEN, kHi0, kEnd, 16>::run(a, x1, naj);
      } else if constexpr (NSMAX == 16 && SMAX <= 16) {
        // supernode rows fill DPP row 0, separator rows start DPP row 1.  L[c][J] (c < 16) is
        // lane c of row 0: with row 0 mirrored into row 1 a row_newbcast DPP operand delivers it
        // to both rows; L[sep c][J] is lane c of row 1, only row 1 needs the trailing block.
        double x = EvenRowsToOddRows(a[J]);
        double naj = -a[J];
        DppOperandFence(x, naj, a[J]);
        DppColumns<LEN, J + 1, (J + 2 < NSMAX ? J + 2 : NSMAX), 0>::run(a, x, naj);
        next_pivot();
        DppColumns<LEN, J + 2, NSMAX, 0>::run(a, x, naj);
        DppColumns<LEN, NSMAX, NSMAX + SMAX, NSMAX>::run(a, a[J], naj);
      } else {
        if constexpr (J + 1 < NSMAX + SMAX) a[J + 1] = fma(-ReadLane(a[J], J + 1), a[J], a[J + 1]);
        next_pivot();
#pragma unroll
        for (int c = J + 2; c < NSMAX + SMAX; c++) a[c] = fma(-ReadLane(a[J], c), a[J], a[c]);
      }
#pragma unroll
      for (int q = 0; q < NRHS; q++) {
        const double yj = ReadLane(a[RB + q], J) * inv;
        if (lane > J)
          a[RB + q] = fma(-yj, a[J], a[RB + q]);
        else if (lane == J)
          a[RB + q] = yj;
      }
      ElimSteps<NSMAX, SMAX, J + 1, NRHS, CHECK>::step(a, lane, bad, root1, inv1, ns);
    }
  }
};

}  // namespace cxk
