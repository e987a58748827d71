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

// ---- the software-pipelined step of the two-row shapes (ElimSteps below: 16 < NSMAX + SMAX <= 32, the
// panel over DPP rows 0 and 1).
//
// A lone wavefront pays an issue slot for every wait state the compiler pads with s_nop, and the head of
// a step used to be one chain of such waits (mask -> select, VALU write -> v_permlane16_swap, VALU write
// -> DPP read, v_readlane -> VALU read of its SGPRs).  So
//  * the mirror of pivot column J + 1 (v_permlane16_swap) is taken from the UNSCALED column as soon as it
//    is final, beside the v_readlane of its diagonal entry and ahead of the reciprocal square root's
//    dependent chain; the head of step J + 1 scales it (mirror(a) * inv == mirror(a * inv) bit for bit,
//    inv is uniform), and lane J + 1 of it is never broadcast;
//  * the mask lane == J + 1 is compared there too, at its one use, and lives in one SGPR pair;
//  * every multiply-add is a volatile asm statement and everything else is pinned between
//    sched_barriers, so the order below is the order issued: the chain's levels alternate with the
//    step's multiply-adds instead of following them.
// Per column the multiply-adds still arrive in pivot order with the same operands: every value is the
// same fma chain, the same bits.

// a[C] -= L[C][J] * a[J]: L[C][J] is lane C of the pivot column -- for C < 16 lane C of x0 (DPP row 0 mirrored
// into row 1), for C >= 16 lane C - 16 of the own DPP row of x1 (NSMAX == 16: of a[J] itself, only row 1 needs
// the trailing block).  The sign rides on the operand (-a[J] is exact: the bits of fma(w, -a[J], a[C])).
template <int NSMAX, int SMAX, int J, int C, int LEN>
__device__ __forceinline__ void ElimFmac(double (&a)[LEN], double x0, double x1) {
  if constexpr (C < 16) {
    asm volatile("v_fmac_f64_dpp %0, %1, -%2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                 : "+v"(a[C])
                 : "v"(x0), "v"(a[J]), "n"(C));
  } else if constexpr (NSMAX == 16) {
    asm volatile("v_fmac_f64_dpp %0, %1, -%1 row_newbcast:%2 row_mask:0xf bank_mask:0xf"
                 : "+v"(a[C])
                 : "v"(a[J]), "n"(C - 16));
  } else {
    asm volatile("v_fmac_f64_dpp %0, %1, -%2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                 : "+v"(a[C])
                 : "v"(x1), "v"(a[J]), "n"(C - 16));
  }
}

// The multiply-adds of step J at list positions [P0, P0 + CNT) that exist (position p: column J + 1 + p; N of them).
template <int NSMAX, int SMAX, int J, int P0, int CNT, int N, int LEN>
__device__ __forceinline__ void ElimIssue(double (&a)[LEN], double x0, double x1) {
  if constexpr (CNT > 0 && P0 < N) {
    ElimFmac<NSMAX, SMAX, J, J + 1 + P0>(a, x0, x1);
    ElimIssue<NSMAX, SMAX, J, P0 + 1, CNT - 1, N>(a, x0, x1);
  }
}

// The lane index behind an opaque zero: a compare of it is not the compare of `lane` the caller may have made
// long before (the compiler would keep ONE mask per pivot alive from there -- 32 to 48 SGPRs, spilled into the
// lanes of a VGPR and read back with two v_readlane per step).
__device__ __forceinline__ int OpaqueLane(int lane) {
  int z;
  asm volatile("s_mov_b32 %0, 0" : "=s"(z));
  return lane + z;
}

// Column J is final: the mask of lane J, its diagonal entry, and its mirror over the DPP rows (Swap16:
// s0 = [r0 r0 r2 r2], s1 = [r1 r1 r3 r3]).  The compare separates the multiply-add that wrote the column from
// its first reader; the v_readlane pair between the two copies and the swaps is the swap's two wait states.
template <int J>
__device__ __forceinline__ double ElimPivotColumn(double v, int lz, unsigned long long& m, double& s0, double& s1) {
  typedef unsigned u2 __attribute__((ext_vector_type(2)));
  __builtin_amdgcn_sched_barrier(0);
  m = __builtin_amdgcn_ballot_w64(lz == J);
  asm volatile("" : : "s"(m));  // (compared HERE: not sunk to its use behind the branch)
  __builtin_amdgcn_sched_barrier(0);
  double c0, c1;
  asm volatile("v_mov_b64 %0, %2\n\tv_mov_b64 %1, %2" : "=&v"(c0), "=&v"(c1) : "v"(v));
  __builtin_amdgcn_sched_barrier(0);
  const double d = ReadLane(v, J);
  __builtin_amdgcn_sched_barrier(0);
  const u2 l = __builtin_amdgcn_permlane16_swap(__double2loint(c0), __double2loint(c1), false, false);
  const u2 h = __builtin_amdgcn_permlane16_swap(__double2hiint(c0), __double2hiint(c1), false, false);
  s0 = __hiloint2double(h.x, l.x);
  s1 = __hiloint2double(h.y, l.y);
  __builtin_amdgcn_sched_barrier(0);
  return d;
}

// Elimination steps J .. NSMAX-1 of FactorSupernodeRows (compile-time recursion: every register
// index, lane select and DPP control is an immediate).
// Step J receives sqrt(d_J) and 1/sqrt(d_J) from step J-1, which starts that dependent chain
// (readlane, v_rsq_f64, two Goldschmidt steps: ~130 cycles on a lone wavefront) as soon as column J
// has taken its own update, so that the chain overlaps the remaining column updates of step J-1
// instead of following them.  Same operations on the same values: results are unchanged.
// The two-row shapes (kPipelined) also receive the mask lane == J and the unscaled mirror of column J
// (ElimPivotColumn, issued by step J-1 ahead of the chain) and issue everything in source order.
// THE HAZARD INVARIANT of that order -- the compiler cannot see that the asm statements are DPP
// instructions and does not count an asm statement as a wait state, so nothing pads for us:
//  1. a DPP operand is read at least two VALU instructions after its last write: the head's products
//     (x0, x1) are followed by exactly the two v_cndmask of the select before the first multiply-add, and
//     a[J] itself, written by that select, is read as a DPP operand no earlier than the second multiply-add
//     (NSMAX == 16, J == 15, where the first one already reads it: an explicit s_nop 1);
//  2. v_permlane16_swap reads its two copies at least two instructions after they were written: the
//     two v_readlane of the diagonal entry stand between the copies and the swaps;
//  3. v_readlane reads column J + 1 at least one instruction after the multiply-add that wrote it: the
//     compare and the two copies stand between;
//  4. v_rsq_f64 reads v_readlane's SGPRs at least two instructions later: the two swaps stand between.
// Whoever reorders the statements of step() or ElimPivotColumn() keeps these four distances.
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
      if constexpr (kPipelined) {
        unsigned long long m;
        double s0, s1;
        const int lz = OpaqueLane(lane);
        const double d = ElimPivotColumn<0>(a[0], lz, m, s0, s1);
        if constexpr (CHECK) bad |= !(d > 0.0);
        double root, inv;
        SqrtAndInverse(d, root, inv);
        step(a, lane, bad, root, inv, ns, lz, m, s0, s1);
      } else {
        const double d = ReadLane(a[0], 0);
        if constexpr (CHECK) bad |= !(d > 0.0);
        double root, inv;
        SqrtAndInverse(d, root, inv);
        step(a, lane, bad, root, inv, ns);
      }
    }
  }
  // The two-row shapes run the software-pipelined step (see above).  m: the mask lane == J; s0 / s1: the
  // unscaled mirror of column J; lz: OpaqueLane.
  static constexpr bool kPipelined = NSMAX + SMAX > 16 && NSMAX + SMAX <= 32;
  static __device__ __forceinline__ void step(double (&a)[LEN], int lane, bool& bad, double root, double inv, int ns,
                                              int lz = 0, unsigned long long m = 0, double s0 = 0.0, double s1 = 0.0) {
    if constexpr (kPipelined && J < NSMAX) {
      if (J >= ns) return;
      constexpr int N = NSMAX + SMAX - J - 1;  // multiply-adds of the step: columns J + 1 .. (list positions 0 ..)
      // head: a[J] = (lane == J) ? root : a[J] * inv, and the mirror scaled
      const double x0 = s0 * inv, x1 = s1 * inv, t = a[J] * inv;
      __builtin_amdgcn_sched_barrier(0);  // (the select: the two wait states between the products and a DPP read of them)
      a[J] = __builtin_amdgcn_inverse_ballot_w64(m) ? root : t;
      __builtin_amdgcn_sched_barrier(0);
      // (NSMAX == 16, J == 15: column 16 reads a[J] itself as a DPP operand, two wait states behind the select)
      if constexpr (NSMAX == 16 && J + 1 >= 16 && N > 0) asm volatile("s_nop 1");
      ElimIssue<NSMAX, SMAX, J, 0, 1, N>(a, x0, x1);  // column J + 1: final for step J + 1
      double root1 = 1.0, inv1 = 1.0, t0 = 0.0, t1 = 0.0;
      unsigned long long m1 = 0;
      if constexpr (J + 1 < NSMAX) {
        const double d1 = ElimPivotColumn<J + 1>(a[J + 1], lz, m1, t0, t1);
        if constexpr (CHECK) bad |= !(d1 > 0.0);
        // SqrtAndInverse(d1), a level of its dependent chain at a time between the step's multiply-adds
#define CXK_ELIM_FILL(P0, CNT)                      \
  __builtin_amdgcn_sched_barrier(0);                \
  ElimIssue<NSMAX, SMAX, J, P0, CNT, N>(a, x0, x1); \
  __builtin_amdgcn_sched_barrier(0)
        const double r0 = __builtin_amdgcn_rsq(d1);
        CXK_ELIM_FILL(1, 2);
        double g = d1 * r0, hh = 0.5 * r0;
        CXK_ELIM_FILL(3, 2);
        double e = fma(-hh, g, 0.5);
        CXK_ELIM_FILL(5, 2);
        g = fma(g, e, g);
        hh = fma(hh, e, hh);
        CXK_ELIM_FILL(7, 2);
        e = fma(-hh, g, 0.5);
        CXK_ELIM_FILL(9, 2);
        g = fma(g, e, g);
        hh = fma(hh, e, hh);
        CXK_ELIM_FILL(11, 2);
        const double res = fma(-g, g, d1);
        inv1 = hh + hh;
        CXK_ELIM_FILL(13, 2);
        root1 = fma(res, hh, g);
        CXK_ELIM_FILL(15, 64);
#undef CXK_ELIM_FILL
        asm volatile("" : : "v"(root1), "v"(inv1));  // (the chain stays HERE: not sunk behind the branch of step J + 1)
      } else {
        ElimIssue<NSMAX, SMAX, J, 1, 64, N>(a, x0, x1);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int q = 0; q < NRHS; q++) {
        const double yj = ReadLane(a[RB + q], J) * inv;
        if (lane > J)
          a[RB + q] = fma(-yj, a[J], a[RB + q]);
        else if (lane == J)
          a[RB + q] = yj;
      }
      ElimSteps<NSMAX, SMAX, J + 1, NRHS, CHECK>::step(a, lane, bad, root1, inv1, ns, lz, m1, t0, t1);
    } else if constexpr (J < NSMAX) {
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
