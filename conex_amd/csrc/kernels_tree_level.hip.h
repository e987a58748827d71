// The level kernels of the elimination tree: one launch per level, level range, pair of levels or
// chain (tree_*), and the supernodal matrix-vector product of iterative refinement (kkt_matvec).
// Only kkt_tree_launch.hip includes this header: it owns every instance of these templates, and
// kkt_matvec is a plain kernel that must be defined in one translation unit.
#pragma once
#include "tree_supernode.hip.h"

namespace cxk {

// MODE 0: factor (+ forward if rhs), MODE 1: forward only, MODE 2: backward.
// TOP = false: one level per launch, positions [base0, base0 + cnt0) of the level-ordered
// records, one wavefront per supernode.
// TOP = true: a RANGE of `nl` consecutive levels per launch.  Workgroup g sweeps one connected
// piece of the elimination forest restricted to those levels (a subtree, or the whole top of
// the tree): its records are stored level by level, wg_lev[g * (nl + 1) + l] is the first
// position of its level l.  Levels inside the workgroup are separated by a workgroup barrier
// instead of a kernel boundary; MODE 0/1 walk them upwards and (then_backward) straight back
// down, MODE 2 walks them downwards.  The records of the piece are prefetched into LDS with one
// load at kernel start, so a level step pays one memory round trip (its data) instead of two.
// The kernel is specialised per (MODE, TOP) so that each instance keeps only the plan fields it
// uses in SGPRs.

template <int MODE, bool TOP>
__global__ void __launch_bounds__(512)
tree_sweep(FactorPlan P, const SnRec* __restrict__ recs, const int* __restrict__ wg_lev, int base0,
           int cnt0, int nl, int then_backward, double* __restrict__ slab, double* __restrict__ rhs,
           int* __restrict__ fail, int lds_per_wave) {
  extern __shared__ double lds[];
  __shared__ int s_rec[TOP ? kRangeMaxRecs * 32 : 32];
  // wave-uniform values are forced into SGPRs: otherwise every loop bound / lane select below
  // is treated as divergent (waterfall loops around v_readlane, vector address arithmetic)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  double* my = lds + (size_t)wave * lds_per_wave;
  CXK_STAMP_SELECT(TOP ? 1 : 0, MODE);
  CXK_STAMP(6);
  CXK_STAMPB(0);
  const int* lp = nullptr;
  int first = base0;
  bool prefetched = false;
  if constexpr (TOP) {
    lp = wg_lev + (size_t)blockIdx.x * (nl + 1);
    first = lp[0];
    const int nrec = lp[nl] - first;
    prefetched = nrec <= kRangeMaxRecs;  // a long narrow top (chain-shaped trees) reads from HBM
    if (prefetched) {
      const int* src = reinterpret_cast<const int*>(recs + first);
      for (int q = threadIdx.x; q < nrec * 32; q += blockDim.x) s_rec[q] = src[q];
    }
    __syncthreads();
  } else {
    nl = 1;
    then_backward = 0;
  }
  auto load_rec = [&](int pos) -> SnRec {
    if (TOP && prefetched) return LoadRec(reinterpret_cast<const SnRec*>(s_rec), pos - first);
    return LoadRec(recs, pos);
  };
  if constexpr (MODE != 2) {
    for (int l = 0; l < nl; l++) {
      const int base = TOP ? lp[l] : base0;
      const int cnt = TOP ? lp[l + 1] - base : cnt0;
      CXK_STAMP_LEVEL(l);
      for (int idx = (TOP ? 0 : blockIdx.x * nw) + wave; idx < cnt; idx += (TOP ? 1 : gridDim.x) * nw) {
        const SnRec R = load_rec(base + idx);
        const int ns = R.ns, s = R.nsep;
        if constexpr (MODE == 0) {
          if (ns <= 8 && s <= 8)
            FactorSupernodeRows<8, 8>(P, R, slab, rhs, fail, my);
          else if (ns <= 16 && s <= 8)
            FactorSupernodeRows<16, 8>(P, R, slab, rhs, fail, my);
          else if (ns <= 24 && s == 0)
            FactorSupernodeRows<24, 0>(P, R, slab, rhs, fail, my);
          else if (ns <= 24 && s <= 8)
            FactorSupernodeRows<24, 8>(P, R, slab, rhs, fail, my);
          else if (ns <= 32 && s <= 16)
            FactorSupernodeRows<32, 16>(P, R, slab, rhs, fail, my);
          else
            CholSupernodeLds(P, R.p, slab, rhs, fail, my);
        } else {
          if (ns <= 64)
            ForwardSupernodeWave(P, R.p, slab, rhs, my);
          else
            ForwardSupernodeLds(P, R.p, slab, rhs, my);
        }
      }
      if constexpr (TOP) __syncthreads();
    }
  }
  if (MODE == 2 || (TOP && then_backward)) {
    for (int l = nl - 1; l >= 0; l--) {
      const int base = TOP ? lp[l] : base0;
      const int cnt = TOP ? lp[l + 1] - base : cnt0;
      for (int idx = (TOP ? 0 : blockIdx.x * nw) + wave; idx < cnt; idx += (TOP ? 1 : gridDim.x) * nw) {
        const SnRec R = load_rec(base + idx);
        const int ns = R.ns, s = R.nsep;
        if (ns <= 8 && s <= 8)
          BackwardSupernodeRows<8, 8>(P, R, slab, rhs);
        else if (ns <= 16 && s <= 8)
          BackwardSupernodeRows<16, 8>(P, R, slab, rhs);
        else if (ns <= 24 && s <= 8)
          BackwardSupernodeRows<24, 8>(P, R, slab, rhs);
        else if (ns <= 32 && s <= 16)
          BackwardSupernodeRows<32, 16>(P, R, slab, rhs);
        else if (ns <= 64)
          BackwardSupernodeWave(P, R.p, slab, rhs, my);
        else
          BackwardSupernodeLds(P, R.p, slab, rhs, my);
      }
      if constexpr (TOP) __syncthreads();
    }
  }
  CXK_STAMP(7);
  CXK_STAMPB(5);
}

// ---------------------------------------------------------------------------------------
// One factor level whose supernodes all fit ONE register shape (NSMAX, SMAX): the same step as
// tree_sweep<0, false>, compiled for that shape alone.  The generic kernel carries every shape's
// elimination plus the LDS fallback and pays for it in scalar-register spills on the path of each
// shape; a level of a regular clique tree (all of BASELINE config 4) takes this kernel instead.
// ---------------------------------------------------------------------------------------
template <int NSMAX, int SMAX, bool RHS>
__global__ void __launch_bounds__(256)
tree_factor_level(FactorPlan P, const SnRec* __restrict__ recs, int base0, int cnt0,
                  double* __restrict__ slab, double* __restrict__ rhs, int* __restrict__ fail,
                  int lds_per_wave) {
  extern __shared__ double lds[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  double* my = lds + (size_t)wave * lds_per_wave;
  const int idx = blockIdx.x * nw + wave;
  CXK_STAMP_SELECT(0, 0);
  CXK_STAMP(6);
  if (idx >= cnt0) return;
  const SnRec R = LoadRec(recs, base0 + idx);
  FactorSupernodeLean<NSMAX, SMAX, RHS>(P, R, slab, rhs, fail, my);
  CXK_STAMP(7);
}

// The first factor level with the assembly folded in: workgroups [0, fwgs) factor supernodes
// whose panels come straight from the Schur blocks (AsmRec), the others run the gather of
// everything else (slab entries of the levels above, their right-hand side, <w,c>, <c,Qc>) --
// needed by the NEXT level's launch only.
template <int NSMAX, int SMAX, bool RHS>
__global__ void __launch_bounds__(256)
tree_factor_level_asm(FactorPlan P, const SnRec* __restrict__ recs, int base0, int cnt0,
                      double* __restrict__ slab, double* __restrict__ rhs, int* __restrict__ fail,
                      int lds_per_wave, AsmIn ai, GatherArgs ga, int fwgs) {
  extern __shared__ double lds[];
  if ((int)blockIdx.x >= fwgs) {
    GatherBody(ga, blockIdx.x - fwgs, gridDim.x - fwgs);
    return;
  }
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  double* my = lds + (size_t)wave * lds_per_wave;
  const int idx = blockIdx.x * nw + wave;
  if (idx >= cnt0) return;
  const int lane = threadIdx.x & 63;
  const int aw2 = reinterpret_cast<const int*>(ai.rec + idx)[lane < 24 ? lane : 0];  // same trip as the record
  const SnRec R = LoadRec(recs, base0 + idx);
  FactorSupernodeLean<NSMAX, SMAX, RHS, true>(P, R, slab, rhs, fail, my, &ai, aw2);
}

// tree_factor_level_asm for a first level of TWO register shapes (programs mixing matrix cones with
// second-order cones: config 5): workgroups [0, blocksA) shape A, [blocksA, fwgs) shape B, the rest
// the gather.  AsmRec q belongs to level position q (segment B follows segment A).
template <int NA, int SA, int NB, int SB>
__global__ void __launch_bounds__(256)
tree_factor_level2_asm(FactorPlan P, const SnRec* __restrict__ recs, int baseA, int cntA, int blocksA,
                       int baseB, int cntB, double* __restrict__ slab, double* __restrict__ rhs,
                       int* __restrict__ fail, int lds_per_wave, AsmIn ai, GatherArgs ga, int fwgs) {
  extern __shared__ double lds[];
  if ((int)blockIdx.x >= fwgs) {
    GatherBody(ga, blockIdx.x - fwgs, gridDim.x - fwgs);
    return;
  }
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  double* my = lds + (size_t)wave * lds_per_wave;
  const int lane = threadIdx.x & 63;
  if ((int)blockIdx.x < blocksA) {
    const int idx = blockIdx.x * nw + wave;
    if (idx >= cntA) return;
    const int aw2 = reinterpret_cast<const int*>(ai.rec + idx)[lane < 24 ? lane : 0];
    const SnRec R = LoadRec(recs, baseA + idx);
    FactorSupernodeLean<NA, SA, true, true>(P, R, slab, rhs, fail, my, &ai, aw2);
  } else {
    const int idx = (blockIdx.x - blocksA) * nw + wave;
    if (idx >= cntB) return;
    const int aw2 = reinterpret_cast<const int*>(ai.rec + cntA + idx)[lane < 24 ? lane : 0];
    const SnRec R = LoadRec(recs, baseB + idx);
    FactorSupernodeLean<NB, SB, true, true>(P, R, slab, rhs, fail, my, &ai, aw2);
  }
}

// The backward step of one level, same specialisation (no LDS).
template <int NSMAX, int SMAX>
__global__ void __launch_bounds__(256)
tree_backward_level(const SnRec* __restrict__ recs, int base0, int cnt0, const double* __restrict__ slab,
                    double* __restrict__ rhs) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  const int idx = blockIdx.x * nw + wave;
  if (idx >= cnt0) return;
  CXK_STAMP_SELECT(0, 2);
  CXK_STAMPB(0);
  const SnRec R = LoadRec(recs, base0 + idx);
  BackwardSupernodeLean<NSMAX, SMAX>(R, slab, rhs);
  CXK_STAMPB(5);
}

template <int NSMAX, int SMAX>
__global__ void __launch_bounds__(256)
tree_forward_level(FactorPlan P, const SnRec* __restrict__ recs, int base0, int cnt0,
                   const double* __restrict__ slab, double* __restrict__ rhs, RhsIn ri) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  const int idx = blockIdx.x * nw + wave;
  if (idx >= cnt0) return;
  const SnRec R = LoadRec(recs, base0 + idx);
  ForwardSupernodeLean<NSMAX, SMAX>(P, R, slab, rhs, ri);
}

template <int NA, int SA, int NB, int SB>
__global__ void __launch_bounds__(256)
tree_forward_level2(FactorPlan P, const SnRec* __restrict__ recs, int baseA, int cntA, int blocksA,
                    int baseB, int cntB, const double* __restrict__ slab, double* __restrict__ rhs, RhsIn ri) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  if ((int)blockIdx.x < blocksA) {
    const int idx = blockIdx.x * nw + wave;
    if (idx >= cntA) return;
    const SnRec R = LoadRec(recs, baseA + idx);
    ForwardSupernodeLean<NA, SA>(P, R, slab, rhs, ri);
  } else {
    const int idx = (blockIdx.x - blocksA) * nw + wave;
    if (idx >= cntB) return;
    const SnRec R = LoadRec(recs, baseB + idx);
    ForwardSupernodeLean<NB, SB>(P, R, slab, rhs, ri);
  }
}

// Two segments of one level in ONE launch (the supernodes of a level are independent): workgroups
// [0, blocksA) run shape A, the rest shape B.  Programs that mix small cones (second-order cones:
// shape <8,8>) with matrix cones have two shapes on every level; two launches would serialise.
template <int NA, int SA, int NB, int SB, bool RHS>
__global__ void __launch_bounds__(256)
tree_factor_level2(FactorPlan P, const SnRec* __restrict__ recs, int baseA, int cntA, int blocksA,
                   int baseB, int cntB, double* __restrict__ slab, double* __restrict__ rhs,
                   int* __restrict__ fail, int lds_per_wave) {
  extern __shared__ double lds[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  double* my = lds + (size_t)wave * lds_per_wave;
  if ((int)blockIdx.x < blocksA) {
    const int idx = blockIdx.x * nw + wave;
    if (idx >= cntA) return;
    const SnRec R = LoadRec(recs, baseA + idx);
    FactorSupernodeLean<NA, SA, RHS>(P, R, slab, rhs, fail, my);
  } else {
    const int idx = (blockIdx.x - blocksA) * nw + wave;
    if (idx >= cntB) return;
    const SnRec R = LoadRec(recs, baseB + idx);
    FactorSupernodeLean<NB, SB, RHS>(P, R, slab, rhs, fail, my);
  }
}

template <int NA, int SA, int NB, int SB>
__global__ void __launch_bounds__(256)
tree_backward_level2(const SnRec* __restrict__ recs, int baseA, int cntA, int blocksA, int baseB, int cntB,
                     const double* __restrict__ slab, double* __restrict__ rhs) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  if ((int)blockIdx.x < blocksA) {
    const int idx = blockIdx.x * nw + wave;
    if (idx >= cntA) return;
    const SnRec R = LoadRec(recs, baseA + idx);
    BackwardSupernodeLean<NA, SA>(R, slab, rhs);
  } else {
    const int idx = (blockIdx.x - blocksA) * nw + wave;
    if (idx >= cntB) return;
    const SnRec R = LoadRec(recs, baseB + idx);
    BackwardSupernodeLean<NB, SB>(R, slab, rhs);
  }
}

// Two consecutive levels of the way DOWN in one launch.  Workgroup g (nine wavefronts) owns one
// supernode of the upper level and the supernodes of the lower level that read its solution
// (BackPairEntry; the host orders a level so that they are consecutive): wavefront 0 solves the
// parent while wavefronts 1 .. 8 already fetch their children's panels, the workgroup barrier
// publishes the parent's solution, the children finish.  Lower-level supernodes that read nothing
// of the upper level ride in parentless workgroups.  Same device function as tree_backward_level
// on the same records: same bits, one launch and one cold start fewer per pair.
template <int NP, int SP, int NC, int SC>
__global__ void __launch_bounds__(576)
tree_backward_pair(const SnRec* __restrict__ recs, const BackPairEntry* __restrict__ tab,
                   const double* __restrict__ slab, double* __restrict__ rhs) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const BackPairEntry e = tab[blockIdx.x];
  const bool with_parent = e.parent >= 0;
  if (wave == 0) {
    if (!with_parent) return;
    const SnRec R = LoadRec(recs, e.parent);
    BackwardSupernodeLean<NP, SP>(R, slab, rhs);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __syncthreads();
    return;
  }
  int i = wave - 1;
  if (i >= e.count) {
    if (with_parent) __syncthreads();  // every wavefront of the workgroup meets the one barrier
    return;
  }
  {
    const SnRec R = LoadRec(recs, e.first + i);
    BackwardSupernodeLeanSync<NC, SC, true>(R, slab, rhs, [&] {
      if (with_parent) {
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      }
    });
  }
  for (i += 8; i < e.count; i += 8) {
    const SnRec R = LoadRec(recs, e.first + i);
    BackwardSupernodeLeanSync<NC, SC, true>(R, slab, rhs, [] {});
  }
}

// The CHAIN at the top of the tree -- trailing levels of exactly one supernode each (the root and
// what leads to it) -- as one launch of ONE wavefront: steps up (MODE 0 factor + forward, MODE 1
// forward) and straight back down.  Consecutive steps are dependent anyway, so a launch per level
// buys nothing here; the wavefront passes its published values to itself through memory
// (workgroup-scope fence between steps: one CU, one L1).  Shapes A and B cover the chain's
// supernodes.  Dependent memory round trips are what a step costs (~1.2 us each), so: the
// records come from consecutive positions (no table look-up), each is fetched while the step
// before it runs and kept in LDS for the way down, and the root turns around in registers.

template <int MODE, int NA, int SA, int NB, int SB>
__global__ void __launch_bounds__(64)
tree_chain_lean(FactorPlan P, const SnRec* __restrict__ recs, int pos0, int n, double* __restrict__ slab,
                double* __restrict__ rhs, int* __restrict__ fail, RhsIn ri) {
  extern __shared__ double lds[];
  // One supernode per level: the chain's records are consecutive in level order (pos0 ..).  Each
  // record is in flight while the step before it runs; the last kChainRing of them stay in LDS for
  // the way back down, the ones below are fetched again, one step ahead as on the way up (a chain
  // may be thousands of levels long: BASELINE config 3 as the reference arranges it).
  constexpr int IMG = 65 * (NA > NB ? NA : NB);  // RootBackward's image (>= the pull image of 64 columns)
  int* rec_lds = reinterpret_cast<int*>(lds + IMG);
  const int ntop = n;  // upward steps
  const int lane = threadIdx.x & 63;
#if defined(CXK_DEBUG_STAMPS) || defined(CXK_CHAIN_STAMPS)
  long long tstamp[8];  // held in registers, written once at the end: no memory traffic in between
  int nstamp = 0;
  tstamp[nstamp++] = __builtin_amdgcn_s_memtime();
#endif
  int wnext = LoadRecWord(recs, pos0);
  for (int q = 0; q < n; q++) {
    const int w = wnext;
    if (q + 1 < n) wnext = LoadRecWord(recs, pos0 + q + 1);
    if (lane < 32) rec_lds[32 * (q & (kChainRing - 1)) + lane] = w;
    const SnRec R = DecodeRec(w);
    const int shape = RegisterShape(R.ns, R.nsep);
    const bool isA = shape == (NA << 8 | SA);
    // the last step is the root (no separator): solved backward from the registers of its
    // upward step (shape B; a root of another shape takes the steps through memory like the rest)
    const bool root = q + 1 == n && shape == (NB << 8 | SB) && R.nsep == 0;
    if constexpr (MODE == 0) {
      if (root)
        FactorSupernodeLean<NB, SB, true, false, true>(P, R, slab, rhs, fail, lds);
      else if (isA)
        FactorSupernodeLean<NA, SA, true>(P, R, slab, rhs, fail, lds);
      else
        FactorSupernodeLean<NB, SB, true>(P, R, slab, rhs, fail, lds);
    } else {
      if (root)
        ForwardSupernodeLean<NB, SB, true>(P, R, slab, rhs, ri, lds);
      else if (isA)
        ForwardSupernodeLean<NA, SA>(P, R, slab, rhs, ri);
      else
        ForwardSupernodeLean<NB, SB>(P, R, slab, rhs, ri);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
#if defined(CXK_DEBUG_STAMPS) || defined(CXK_CHAIN_STAMPS)
    if (nstamp < 7) tstamp[nstamp++] = __builtin_amdgcn_s_memtime();
#endif
    if (root) n--;  // done with the root: the way down starts below it
  }
  WaveSync();
  const int first_cached = ntop - kChainRing;  // records q >= first_cached are in the ring
  int wdown = (n - 1 >= 0 && n - 1 < first_cached) ? LoadRecWord(recs, pos0 + n - 1) : 0;
  for (int q = n - 1; q >= 0; q--) {
    const int wq = q >= first_cached ? rec_lds[32 * (q & (kChainRing - 1)) + (lane & 31)] : wdown;
    if (q - 1 >= 0 && q - 1 < first_cached) wdown = LoadRecWord(recs, pos0 + q - 1);
    const SnRec R = DecodeRec(wq);
    const bool isA = RegisterShape(R.ns, R.nsep) == (NA << 8 | SA);
    if (isA)
      BackwardSupernodeLean<NA, SA>(R, slab, rhs);
    else
      BackwardSupernodeLean<NB, SB>(R, slab, rhs);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
#if defined(CXK_DEBUG_STAMPS) || defined(CXK_CHAIN_STAMPS)
    if (nstamp < 8) tstamp[nstamp++] = __builtin_amdgcn_s_memtime();
#endif
  }
#if defined(CXK_DEBUG_STAMPS) || defined(CXK_CHAIN_STAMPS)
  if (threadIdx.x == 0)
    for (int i = 0; i < 8; i++) g_cxk_stamp[80 + i] = i < nstamp ? tstamp[i] : 0;
#endif
}

// ---------------------------------------------------------------------------------------
// Mid-size supernodes (ns > 32 or s > 16, panel still LDS resident): ONE WORKGROUP per
// supernode.  Same arithmetic as the register kernels -- right-looking elimination with
// reciprocal scaling and fma updates, published updates as fma chains over the solved panel --
// executed block-wide on an LDS copy [diag ns x ns | off ns x s | rhs ns], two barriers per column.
// MODE as in tree_sweep.  grid = supernodes of the level (positions base0 ..).
// ---------------------------------------------------------------------------------------
template <int MODE>
__global__ void __launch_bounds__(256)
tree_sweep_block(FactorPlan P, int base0, double* __restrict__ slab, double* __restrict__ rhs,
                 int* __restrict__ fail) {
  extern __shared__ double lds[];
  __shared__ int s_bad;
  const SnRec R = LoadRec(P.rec, base0 + blockIdx.x);
  const int ns = R.ns, s = R.nsep, tid = threadIdx.x, nt = blockDim.x;
  double* D = slab + R.diag_off;
  double* B = slab + R.offd_off;
  double* sD = lds;
  double* sB = sD + ns * ns;
  double* sb = sB + ns * s;
  if (tid == 0) s_bad = 0;
  if (MODE == 2) {
    // b <- L^{-T} (b - sum_c off[:,c] y[sep c]); separator terms in the reference's order
    for (int q = tid; q < ns * ns; q += nt) sD[q] = D[q];
    for (int i = tid; i < ns; i += nt) {
      double acc = rhs[R.start + i];
      for (int q = R.bs_beg; q < R.bs_end; q++) acc -= B[i + (size_t)P.bs_c[q] * ns] * rhs[P.bs_row[q]];
      sb[i] = acc;
    }
    __syncthreads();
    for (int k = ns - 1; k >= 0; k--) {
      if (tid == 0) sb[k] = sb[k] * (1.0 / sD[k + k * ns]);
      __syncthreads();
      const double yk = sb[k];
      for (int i = tid; i < k; i += nt) sb[i] = fma(-sD[k + i * ns], yk, sb[i]);
      __syncthreads();
    }
    for (int i = tid; i < ns; i += nt) rhs[R.start + i] = sb[i];
    return;
  }
  const bool with_matrix = MODE == 0;
  const bool with_rhs = rhs != nullptr;
  {
    const int nd = ns * ns, total = nd + ns * s;
    for (int q = tid; q < total; q += nt) lds[q] = q < nd ? D[q] : B[q - nd];
    if (with_rhs)
      for (int i = tid; i < ns; i += nt) sb[i] = rhs[R.start + i];
  }
  __syncthreads();
  if (with_matrix)
    for (int t = R.tg_beg + tid; t < R.tg_end; t += nt) {
      const int loc = P.tg_loc[t];
      double acc = lds[loc];
      const int q1 = P.tr_ptr[t + 1];
      for (int q = P.tr_ptr[t]; q < q1; q++) acc -= P.upd[P.tr_src[q]];
      lds[loc] = acc;
    }
  if (with_rhs)
    for (int i = tid; i < ns; i += nt) {
      double acc = sb[i];
      const int q1 = P.fs_ptr[R.start + i + 1];
      for (int q = P.fs_ptr[R.start + i]; q < q1; q++) acc -= P.updb[P.fs_src[q]];
      sb[i] = acc;
    }
  __syncthreads();
  // extra columns carried along: off block (factor sweep only; solved already otherwise), rhs
  const int ext = s + (with_rhs ? 1 : 0), c0 = with_matrix ? 0 : s;
  for (int k = 0; k < ns; k++) {
    double inv;
    if (with_matrix) {
      const double d = sD[k + k * ns];
      double root;
      SqrtAndInverse(d, root, inv);
      if (!(d > 0.0) && tid == 0) s_bad = 1;
      __syncthreads();  // everybody has read the pivot
      for (int i = k + tid; i < ns; i += nt) sD[i + k * ns] = (i == k) ? root : sD[i + k * ns] * inv;
    } else {
      inv = 1.0 / sD[k + k * ns];
    }
    for (int c = c0 + tid; c < ext; c += nt) {
      double* col = c < s ? sB + c * ns : sb;
      col[k] = col[k] * inv;
    }
    __syncthreads();
    const int rows = ns - k - 1;
    const int dcols = with_matrix ? rows : 0;
    for (int idx = tid; idx < rows * (dcols + ext - c0); idx += nt) {
      const int i = k + 1 + idx % rows, cc = idx / rows;
      const double lik = sD[i + k * ns];
      if (cc < dcols) {
        const int j = k + 1 + cc;
        if (j <= i) sD[i + j * ns] = fma(-lik, sD[j + k * ns], sD[i + j * ns]);
      } else {
        const int c = c0 + cc - dcols;
        double* col = c < s ? sB + c * ns : sb;
        col[i] = fma(-lik, col[k], col[i]);
      }
    }
    __syncthreads();
  }
  if (with_matrix && s_bad) {
    if (tid == 0) atomicExch(fail, 1);
    return;
  }
  if (with_matrix) {
    for (int q = tid; q < ns * ns; q += nt)
      if (q % ns >= q / ns) D[q] = sD[q];
    for (int q = tid; q < ns * s; q += nt) B[q] = sB[q];
    const int* dst = P.pub_dst + R.upd_off;
    const int npairs = s * (s + 1) / 2;
    for (int t = tid; t < npairs; t += nt) {
      int k = 0, rem = t;
      while (rem >= s - k) {
        rem -= s - k;
        k++;
      }
      const int j = k + rem;
      double dot = 0;
      for (int i = 0; i < ns; i++) dot = fma(sB[i + k * ns], sB[i + j * ns], dot);
      P.upd[dst[t]] = dot;
    }
  }
  if (with_rhs) {
    for (int i = tid; i < ns; i += nt) rhs[R.start + i] = sb[i];
    const int* dst = P.pubb_dst + R.updb_off;
    for (int c = tid; c < s; c += nt) {
      double dot = 0;
      for (int i = 0; i < ns; i++) dot = fma(sB[i + c * ns], sb[i], dot);
      P.updb[dst[c]] = dot;
    }
  }
}

// ---------------------------------------------------------------------------------------
// LDLT path (programs with equality constraints: multipliers make the KKT matrix indefinite).
// Reference: BlockLDLTInPlace block_triangular_operations.cc:315-349 over Eigen::RLDLT
// (RLDLT.h:298-431: diagonal pivoting on the largest |diagonal|, left-looking column update,
// pivots with |d| <= 1e-9 clamped to +-1e-9), solves ApplyBlockInverseOfMD :265-299 and
// ApplyBlockInverseOfMTranspose :222-263.  One workgroup per supernode, panel in LDS
// [diag ns x ns | off ns x s | rhs ns | temp ns]; `tr` holds the transpositions (local indices)
// of every supernode by first permuted index.  Published updates:
//   U[k][j] = sum_r (D_r off[r][k]) off[r][j]   with off = D^-1 L^-1 P off
//   t[c]    = sum_r off[r][c] b_r               with b = L^-1 P b (D^-1 is applied afterwards)
// ---------------------------------------------------------------------------------------
// HBM: the panel image lives in `ws` (global memory) instead of LDS -- supernodes beyond LDS, one
// workgroup of 1024 threads each, the same operations in the same order (a workgroup barrier orders
// its threads' global accesses as it orders their LDS accesses); the extra columns (off block,
// right-hand side) are then swept by all threads together, column step by column step, instead of
// one thread per column.  Slow (every step is a round trip to L2) but complete: the blocked LDLT with
// the reference's pivot rule needs the whole trailing diagonal at every step.
template <int MODE, bool HBM = false>
__global__ void __launch_bounds__(HBM ? 1024 : 256)
tree_sweep_block_ldlt(FactorPlan P, int base0, double* __restrict__ slab, double* __restrict__ rhs,
                      int* __restrict__ tr_all, int* __restrict__ regularized, double* __restrict__ ws = nullptr) {
  extern __shared__ double lds_dyn[];
  double* lds = HBM ? ws : lds_dyn;
  __shared__ double s_val[16];
  __shared__ int s_idx[16];
  __shared__ int s_piv;
  const SnRec R = LoadRec(P.rec, base0 + blockIdx.x);
  const int ns = R.ns, s = R.nsep, tid = threadIdx.x, nt = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6;
  double* D = slab + R.diag_off;
  double* B = slab + R.offd_off;
  double* sD = lds;
  double* sB = sD + ns * ns;
  double* sb = sB + ns * s;
  double* temp = sb + ns;
  int* str = reinterpret_cast<int*>(temp + ns);  // LDS copy of the transpositions
  int* tr = tr_all + R.start;
  if (MODE == 2) {
    for (int q = tid; q < ns * ns; q += nt) sD[q] = D[q];
    for (int i = tid; i < ns; i += nt) {
      double acc = rhs[R.start + i];
      for (int q = R.bs_beg; q < R.bs_end; q++) acc -= B[i + (size_t)P.bs_c[q] * ns] * rhs[P.bs_row[q]];
      sb[i] = acc;
    }
    __syncthreads();
    for (int k = ns - 1; k >= 0; k--) {  // unit-lower-transposed solve
      const double yk = sb[k];
      for (int i = tid; i < k; i += nt) sb[i] = fma(-sD[k + i * ns], yk, sb[i]);
      __syncthreads();
    }
    if (tid == 0)
      for (int k = ns - 1; k >= 0; k--) {  // P^T
        const int t = tr[k];
        if (t != k) {
          const double v = sb[k];
          sb[k] = sb[t];
          sb[t] = v;
        }
      }
    __syncthreads();
    for (int i = tid; i < ns; i += nt) rhs[R.start + i] = sb[i];
    return;
  }
  const bool with_matrix = MODE == 0;
  const bool with_rhs = rhs != nullptr;
  {
    const int nd = ns * ns, total = nd + ns * s;
    for (int q = tid; q < total; q += nt) lds[q] = q < nd ? D[q] : B[q - nd];
    if (with_rhs)
      for (int i = tid; i < ns; i += nt) sb[i] = rhs[R.start + i];
  }
  if (!with_matrix)
    for (int i = tid; i < ns; i += nt) str[i] = tr[i];
  __syncthreads();
  if (with_matrix)
    for (int t = R.tg_beg + tid; t < R.tg_end; t += nt) {
      const int loc = P.tg_loc[t];
      double acc = lds[loc];
      const int q1 = P.tr_ptr[t + 1];
      for (int q = P.tr_ptr[t]; q < q1; q++) acc -= P.upd[P.tr_src[q]];
      lds[loc] = acc;
    }
  if (with_rhs)
    for (int i = tid; i < ns; i += nt) {
      double acc = sb[i];
      const int q1 = P.fs_ptr[R.start + i + 1];
      for (int q = P.fs_ptr[R.start + i]; q < q1; q++) acc -= P.updb[P.fs_src[q]];
      sb[i] = acc;
    }
  __syncthreads();
  if (with_matrix) {
    if (ns == 1) {  // RLDLT.h:311-330: clamps without reporting
      if (tid == 0) {
        if (fabs(sD[0]) < 1e-9) sD[0] = sD[0] < 0 ? -1e-9 : 1e-9;
        tr[0] = 0;
        str[0] = 0;
      }
      __syncthreads();
    } else {
      for (int k = 0; k < ns; k++) {
        // first largest |diagonal| of the trailing part
        double best = -1.0;
        int bi = k;
        for (int i = k + tid; i < ns; i += nt) {
          const double v = fabs(sD[i + i * ns]);
          if (v > best) {
            best = v;
            bi = i;
          }
        }
        for (int off = 32; off > 0; off >>= 1) {
          const double ov = __shfl_xor(best, off, 64);
          const int oi = __shfl_xor(bi, off, 64);
          if (ov > best || (ov == best && oi < bi)) {
            best = ov;
            bi = oi;
          }
        }
        if (lane == 0) {
          s_val[wave] = best;
          s_idx[wave] = bi;
        }
        __syncthreads();
        if (tid == 0) {
          double b = s_val[0];
          int p = s_idx[0];
          for (int w = 1; w < (nt >> 6); w++)
            if (s_val[w] > b || (s_val[w] == b && s_idx[w] < p)) {
              b = s_val[w];
              p = s_idx[w];
            }
          s_piv = p;
          tr[k] = p;
          str[k] = p;
        }
        __syncthreads();
        const int big = s_piv;
        if (big != k) {  // symmetric transposition on the lower triangle (RLDLT.h:343-362)
          for (int j = tid; j < k; j += nt) {
            const double t = sD[k + j * ns];
            sD[k + j * ns] = sD[big + j * ns];
            sD[big + j * ns] = t;
          }
          for (int i = big + 1 + tid; i < ns; i += nt) {
            const double t = sD[i + k * ns];
            sD[i + k * ns] = sD[i + big * ns];
            sD[i + big * ns] = t;
          }
          for (int i = k + 1 + tid; i < big; i += nt) {
            const double t = sD[i + k * ns];
            sD[i + k * ns] = sD[big + i * ns];
            sD[big + i * ns] = t;
          }
          if (tid == 0) {
            const double t = sD[k + k * ns];
            sD[k + k * ns] = sD[big + big * ns];
            sD[big + big * ns] = t;
          }
          __syncthreads();
        }
        for (int j = tid; j < k; j += nt) temp[j] = sD[j + j * ns] * sD[k + j * ns];
        __syncthreads();
        for (int i = k + tid; i < ns; i += nt) {  // row k: the pivot; rows > k: A21
          double acc = 0;
          for (int j = 0; j < k; j++) acc += sD[i + j * ns] * temp[j];
          sD[i + k * ns] -= acc;
        }
        __syncthreads();
        if (tid == 0) {
          const double akk = sD[k + k * ns];
          if (!(fabs(akk) > 1e-9)) {
            sD[k + k * ns] = akk < 0 ? -1e-9 : 1e-9;
            atomicExch(regularized, 1);
          }
        }
        __syncthreads();
        const double akk = sD[k + k * ns];
        for (int i = k + 1 + tid; i < ns; i += nt) sD[i + k * ns] /= akk;
        __syncthreads();
      }
    }
  }
  // extra columns: off block (factor sweep only) and rhs.  One thread per column:
  // P, then the unit-lower solve; off additionally scaled by D^-1.
  const int ext = s + (with_rhs ? 1 : 0), c0 = with_matrix ? 0 : s;
  if constexpr (HBM) {
    for (int c = c0 + tid; c < ext; c += nt) {
      double* col = c < s ? sB + (size_t)c * ns : sb;
      for (int k = 0; k < ns; k++) {
        const int t = str[k];
        if (t != k) {
          const double v = col[k];
          col[k] = col[t];
          col[t] = v;
        }
      }
    }
    __syncthreads();
    const int ncol = ext - c0;
    for (int j = 0; j + 1 < ns; j++) {  // every entry takes its terms in the order of the one-thread sweep
      const int below = ns - j - 1;
      for (int q = tid; q < below * ncol; q += nt) {
        const int c = c0 + q / below, i = j + 1 + q % below;
        double* col = c < s ? sB + (size_t)c * ns : sb;
        col[i] -= sD[i + (size_t)j * ns] * col[j];
      }
      __syncthreads();
    }
    if (with_matrix)
      for (int q = tid; q < ns * s; q += nt) sB[q] = (1.0 / sD[(q % ns) * (size_t)(ns + 1)]) * sB[q];
  } else
  for (int c = c0 + tid; c < ext; c += nt) {
    double* col = c < s ? sB + c * ns : sb;
    for (int k = 0; k < ns; k++) {
      const int t = str[k];
      if (t != k) {
        const double v = col[k];
        col[k] = col[t];
        col[t] = v;
      }
    }
    for (int j = 0; j < ns; j++) {
      const double cj = col[j];
      for (int i = j + 1; i < ns; i++) col[i] -= sD[i + j * ns] * cj;
    }
    if (c < s)
      for (int r = 0; r < ns; r++) col[r] = (1.0 / sD[r + r * ns]) * col[r];
  }
  __syncthreads();
  if (with_matrix) {
    for (int q = tid; q < ns * ns; q += nt)
      if (q % ns >= q / ns) D[q] = sD[q];
    for (int q = tid; q < ns * s; q += nt) B[q] = sB[q];
    const int* dst = P.pub_dst + R.upd_off;
    const int npairs = s * (s + 1) / 2;
    for (int t = tid; t < npairs; t += nt) {
      int k = 0, rem = t;
      while (rem >= s - k) {
        rem -= s - k;
        k++;
      }
      const int j = k + rem;
      double dot = 0;
      for (int r = 0; r < ns; r++) dot += (sD[r + r * ns] * sB[r + k * ns]) * sB[r + j * ns];
      P.upd[dst[t]] = dot;
    }
  }
  if (with_rhs) {
    const int* dst = P.pubb_dst + R.updb_off;
    for (int c = tid; c < s; c += nt) {
      double dot = 0;
      for (int r = 0; r < ns; r++) dot += sB[r + c * ns] * sb[r];
      P.updb[dst[c]] = dot;
    }
    __syncthreads();
    for (int i = tid; i < ns; i += nt) rhs[R.start + i] = (1.0 / sD[i + i * ns]) * sb[i];
  }
}

// ---------------------------------------------------------------------------------------
// Iterative refinement (SupernodalKKTSolver::SolveInPlace, kkt_solver.cc:233-261):
//   y <- y + K^-1 (b - K y)   with K = the assembled matrix, kept in `slab0` by the factor sweep.
// The reference multiplies a dense N x N copy; here K y comes from the supernodal blocks:
// kkt_matvec (one workgroup per supernode) forms  u[sn] = sym(diag) y[sn] + off y[sep]  and
// publishes  t[c] = off[:,c] . y[sn]  into the forward-solve slots' twin `mvb`; refine_residual
// gathers them per row in list order (deterministic) into  r = b - K y, saves y and puts r in its place.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
kkt_matvec(FactorPlan P, const double* __restrict__ slab0, const double* __restrict__ y,
           double* __restrict__ u, double* __restrict__ mvb) {
  const SnRec R = LoadRec(P.rec, blockIdx.x);
  const int ns = R.ns, s = R.nsep, tid = threadIdx.x, nt = blockDim.x;
  const double* D = slab0 + R.diag_off;
  const double* B = slab0 + R.offd_off;
  for (int i = tid; i < ns; i += nt) {
    double acc = 0;
    for (int j = 0; j < ns; j++) acc += (j <= i ? D[i + (size_t)j * ns] : D[j + (size_t)i * ns]) * y[R.start + j];
    for (int q = R.bs_beg; q < R.bs_end; q++) acc += B[i + (size_t)P.bs_c[q] * ns] * y[P.bs_row[q]];
    u[R.start + i] = acc;
  }
  for (int c = tid; c < s; c += nt) {
    double dot = 0;
    for (int i = 0; i < ns; i++) dot += B[i + (size_t)c * ns] * y[R.start + i];
    mvb[P.pubb_dst[R.updb_off + c]] = dot;
  }
}

}  // namespace cxk
