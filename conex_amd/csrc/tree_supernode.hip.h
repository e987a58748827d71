// Device building blocks of the supernodal KKT path, shared by the kernel families (level kernels,
// dense top, big supernodes, block solve, whole-tree launch): the gather body, record loads, and
// the factor / forward / backward steps of one supernode for the level-scheduled block Cholesky /
// LDLT (right-looking inside a supernode, published updates pulled by ancestors) and the block
// triangular solves.  __device__ functions and templates only, no kernel.  Types: kkt_records.h.
// Elimination steps: dense_elim.hip.h.
//
// Reference semantics reproduced here (summation ORDER included, so results do not depend
// on scheduling):
//   SupernodalAssemblerBase::UpdateBlocks (Set/SetLowerTri/Scatter)  supernodal_assembler.cc:113-165
//   SupernodalKKTSolver::Assemble (descending elimination index)     kkt_solver.cc:164-170
//   AssembleSchurComplementResiduals                                 constraint_manager.h:107-124
//   BlockCholeskyInPlace                                             block_triangular_operations.cc:184-219
//   ApplyBlockInverseInPlace / ...OfTransposeInPlace                 block_triangular_operations.cc:114-182
//
// The reference pushes updates through tables of double*; here every target entry PULLS its
// contributions from an index list built on the host in the reference's own order.  Entries
// are owned by exactly one thread, so no atomics are needed and runs are bit-reproducible.
#pragma once
#include "dense_elim.hip.h"
#include "device_utils.h"
#include "kkt_records.h"
#include "kkt_stamps.hip.h"

namespace cxk {

// The gather of workgroup `block` of `nblocks` (assemble_gather, and the gather workgroups that
// ride in the first factor level's launch: tree_factor_level_asm).
__device__ __forceinline__ void GatherBody(const GatherArgs& a, int block, int nblocks) {
  const int64_t gid = block * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)nblocks * blockDim.x;
  const int64_t span = a.T > a.N ? a.T : (int64_t)a.N;
  // slab entries and residual entries are gathered side by side: their loads share the round trips
  for (int64_t t = gid; t < span; t += stride) {
    const bool ht = t < a.T, hp = t < a.N;
    GatherRec g = {0, -1, 0, 0};
    ResidRec r = {-1, 0, 0};
    int var = (int)t;
    if (ht) g = a.rec[t];
    if (hp) r = a.rrec[t];
    if (hp && a.var_idx) var = a.var_idx[t];
    double s = 0, aw = 0, aq = 0, bp = 0;
    if (g.first >= 0) s += a.G[g.first];
    if (r.first >= 0) {
      aw += a.AWc[r.first];
      aq += a.AQcc[r.first];
    }
    if (hp && a.with_rhs) bp = a.b[var];
    for (int k = g.beg; k < g.beg + g.extra; k++) {
      const int64_t q = a.src[k];
      if (q >= 0) s += a.G[q];
    }
    for (int k = r.beg; k < r.beg + r.extra; k++) {
      aw += a.AWc[a.rs_src[k]];
      aq += a.AQcc[a.rs_src[k]];
    }
    if (ht) a.slab[g.dst] = s;
    if (hp) {
      a.AW[var] = aw;
      a.AQc[var] = aq;
      if (a.with_rhs == 1) a.y[var] = a.k * (bp * a.bs + aq * a.cs) - 2 * aw;
      if (a.with_rhs == 2) a.y[var] = a.cb * bp + a.cq * aq + a.cw * aw;
    }
  }
  if (block == 0) {  // <w,c> and <c,Qc>: fixed-order strided partial sums + block sum
    __shared__ double red[8];
    double s0 = 0, s1 = 0;
    for (int i = threadIdx.x; i < a.K; i += blockDim.x) {
      s0 += a.sc[2 * i];
      s1 += a.sc[2 * i + 1];
    }
    s0 = BlockSum(s0, red);
    s1 = BlockSum(s1, red);
    if (threadIdx.x == 0) {
      a.sys_sc[0] = s0;
      a.sys_sc[1] = s1;
      *a.fail = 0;
    }
  }
}

__device__ __forceinline__ int LoadRecWord(const SnRec* __restrict__ rec, int pos) {
  return reinterpret_cast<const int*>(rec + pos)[threadIdx.x & 31];
}
__device__ __forceinline__ SnRec DecodeRec(int w) {
  auto f = [&](int i) { return __builtin_amdgcn_readlane(w, i); };
  auto f64 = [&](int i) { return ((int64_t)f(i + 1) << 32) | (uint32_t)f(i); };
  SnRec R;
  R.p = f(0);
  R.ns = f(1);
  R.nsep = f(2);
  R.start = f(3);
  R.tg_beg = f(4);
  R.tg_end = f(5);
  R.bs_beg = f(6);
  R.bs_end = f(7);
  R.diag_off = f64(8);
  R.offd_off = f64(10);
  R.upd_off = f64(12);
  R.updb_off = f(14);
  R.m = f(15);
  R.ubase = f64(16);
  R.fbase = f(18);
  R.mf = f(19);
  R.nsep_inline = f(20);
#pragma unroll
  for (int q = 0; q < 8; q++) R.sep[q] = f(24 + q);
  return R;
}
__device__ __forceinline__ SnRec LoadRec(const SnRec* __restrict__ rec, int pos) { return DecodeRec(LoadRecWord(rec, pos)); }

// The root of the tree (no separator) solved backward straight from the registers of its upward
// step: the rows of L go through an LDS image with an odd stride (my[65 j + row]) and come back
// as columns; arithmetic and order are BackwardSupernodeLean's, so are the bits.  `y` is the
// forward-solved right-hand side of lane's row.  Needs 65 NSMAX doubles at `my`.
template <int NSMAX, bool DIAG_IN_ROWS, int LEN>
__device__ __forceinline__ double RootBackward(const double (&a)[LEN], double dg, double y, int ns, double* __restrict__ my) {
  const int lane = threadIdx.x & 63;
  const bool active = lane < ns;
#pragma unroll
  for (int j = 0; j < NSMAX; j++) my[65 * j + lane] = a[j];
  WaveSync();
  double col[NSMAX];
#pragma unroll
  for (int k = 0; k < NSMAX; k++) col[k] = my[65 * (active ? lane : 0) + k];
  if constexpr (DIAG_IN_ROWS) dg = my[66 * (active ? lane : 0)];  // a[lane] of the own row
#pragma unroll
  for (int k = 0; k < NSMAX; k++) col[k] = (active && k > lane && k < ns) ? col[k] : 0.0;
  dg = active ? dg : 1.0;
  double acc = active ? y : 0.0;
  const double dinv = 1.0 / dg;
#pragma unroll
  for (int k = NSMAX - 1; k >= 0; k--) {
    if (lane == k) acc *= dinv;
    acc = fma(-col[k], ReadLane(acc, k), acc);  // col[k] is zero for lanes >= k
  }
  return acc;
}

// Stage [diag | off | rhs] of supernode p into the wave's LDS region and apply the published
// updates of its descendants in the reference's order.  Layout: sD ns*ns, sB ns*s, sb ns.
__device__ inline void StageAndPull(const FactorPlan& P, int p, const double* __restrict__ slab,
                                    const double* __restrict__ rhs, double* __restrict__ my,
                                    bool with_matrix) {
  const int lane = threadIdx.x & 63;
  const int ns = __builtin_amdgcn_readfirstlane(P.ns[p]), s = __builtin_amdgcn_readfirstlane(P.nsep[p]);
  const double* D = slab + P.diag_off[p];
  const double* B = slab + P.offd_off[p];
  double* sb = my + ns * ns + ns * s;
  const int st = __builtin_amdgcn_readfirstlane(P.start[p]);
  // copy [diag | off] into LDS; loads are issued in independent batches of 8 so their latencies
  // overlap (a plain copy loop waits for each load before the next one is issued)
  {
    const int nd = ns * ns, total = with_matrix ? nd + ns * s : nd;
    for (int base = 0; base < total; base += 8 * 64) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int q = base + u * 64 + lane;
        v[u] = (q < total) ? (q < nd ? D[q] : B[q - nd]) : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int q = base + u * 64 + lane;
        if (q < total) my[q] = v[u];
      }
    }
  }
  if (rhs)
    for (int r = lane; r < ns; r += 64) sb[r] = rhs[st + r];
  WaveSync();
  if (with_matrix) {
    for (int t = P.tg_ptr[p] + lane; t < P.tg_ptr[p + 1]; t += 64) {
      const int loc = P.tg_loc[t];
      double acc = my[loc];
      const int q1 = P.tr_ptr[t + 1];
#pragma unroll 4
      for (int q = P.tr_ptr[t]; q < q1; q++) acc -= P.upd[P.tr_src[q]];
      my[loc] = acc;
    }
  }
  if (rhs) {
    for (int r = lane; r < ns; r += 64) {
      double acc = sb[r];
      const int q1 = P.fs_ptr[st + r + 1];
#pragma unroll 4
      for (int q = P.fs_ptr[st + r]; q < q1; q++) acc -= P.updb[P.fs_src[q]];
      sb[r] = acc;
    }
  }
  WaveSync();
}

// Publish U[k,j] = off[:,k].off[:,j] and t[c] = off[:,c].b from the LDS copies sB / sb.
__device__ inline void PublishUpdates(const FactorPlan& P, int p, const double* __restrict__ my,
                                      bool with_matrix, bool with_rhs) {
  const int lane = threadIdx.x & 63;
  const int ns = __builtin_amdgcn_readfirstlane(P.ns[p]), s = __builtin_amdgcn_readfirstlane(P.nsep[p]);
  const double* sB = my + ns * ns;
  const double* sb = sB + ns * s;
  if (with_matrix) {
    const int* dst = P.pub_dst + P.upd_off[p];
    const int npairs = s * (s + 1) / 2;
    for (int t = lane; t < npairs; t += 64) {
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
    const int* dst = P.pubb_dst + P.updb_off[p];
    for (int c = lane; c < s; c += 64) {
      double dot = 0;
      for (int i = 0; i < ns; i++) dot = fma(sB[i + c * ns], sb[i], dot);
      P.updb[dst[c]] = dot;
    }
  }
}

// ---------------------------------------------------------------------------------------
// One wavefront factors one supernode, ROW PER LANE, everything in registers with static
// indices and no LDS traffic in the elimination loop:
//   lane r < ns            row r of the diagonal block          a[j] = L[r][j]
//   lane NSMAX + c, c < s  row of separator variable c          a[j] = off[j][c]
//   a[NSMAX + c]           the (initially zero) separator x separator trailing block: after the
//                          ns elimination steps it holds  -U[.,c] = -off[:, .] . off[:, c]
//   a[RB]                  right-hand side column: rows < ns end as the forward-solved b, the
//                          separator rows end as  -t[c] = -off[:,c] . b
// i.e. the Schur update and the forward-solve update this supernode publishes for its ancestors
// fall out of the same right-looking elimination (same fma chains as separate dot products).
// Step j: d = a[j] of lane j (v_readlane, static lane), L_jj = sqrt(d) and 1/L_jj from one
// v_rsq_f64 refined by two Goldschmidt iterations, column j scaled, then for every later column
// c:  a[c] -= L[c][j] * a[j]  with L[c][j] read from lane c.  Entries above the diagonal pick up
// garbage and are never read.  Padding pivots (ns <= j < NSMAX) are identity steps.
// ---------------------------------------------------------------------------------------
template <int NSMAX, int SMAX>
__device__ inline void FactorSupernodeRows(const FactorPlan& P, const SnRec& R,
                                           double* __restrict__ slab, double* __restrict__ rhs,
                                           int* __restrict__ fail, double* __restrict__ my) {
  static_assert(NSMAX + SMAX <= 64, "one lane per panel row");
  constexpr int RB = NSMAX + SMAX;
  const int lane = threadIdx.x & 63;
  const int ns = R.ns, s = R.nsep;
  const bool is_row = lane < ns;
  const int sc = lane - NSMAX;
  const bool is_sep = sc >= 0 && sc < s;
  // panel element (lane, j) lives at base[o0 + j * st]:  D[r + j*ns]  or  B[j + c*ns]
  double* base = slab + R.diag_off;
  const unsigned rel = (unsigned)(R.offd_off - R.diag_off);
  const unsigned o0 = is_row ? (unsigned)lane : (is_sep ? rel + (unsigned)(sc * ns) : 0u);
  const unsigned st = is_row ? (unsigned)ns : 1u;
  const int lim = is_row ? lane + 1 : (is_sep ? ns : 0);  // valid j < lim
  CXK_STAMP(0);
  // ---- one round trip: panel, right-hand side, publish destinations and every value this
  // supernode pulls (dense slots: addresses depend on the record only)
  constexpr int TU = 2, MMAX = 8, MFMAX = 8;
  const int ntg = R.tg_end - R.tg_beg;
  const bool fast_pull = ntg <= 64 * TU && R.m <= MMAX && R.mf <= MFMAX;
  double a[NSMAX + SMAX + 1];
#pragma unroll
  for (int j = 0; j < NSMAX; j++) a[j] = (j < lim) ? base[o0 + j * st] : 0.0;
  a[RB] = (rhs && is_row) ? rhs[R.start + lane] : 0.0;
#pragma unroll
  for (int c = 0; c < SMAX; c++) a[NSMAX + c] = 0.0;
  // The remaining loads are guarded by wave-uniform branches and use clamped (always valid)
  // addresses instead of per-lane predicates: a leaf skips them at the cost of a scalar branch.
  int pdst[SMAX > 0 ? SMAX : 1], pdstb = 0;
#pragma unroll
  for (int c = 0; c < SMAX; c++) pdst[c] = 0;
  if (s > 0) {
    const int k = is_sep ? sc : 0;
    const int* dst = P.pub_dst + R.upd_off + (k * s - k * (k - 1) / 2 - k);
#pragma unroll
    for (int c = 0; c < SMAX; c++) {
      const int cc = c < k ? k : (c < s ? c : s - 1);
      pdst[c] = dst[cc];
    }
    if (rhs) pdstb = P.pubb_dst[R.updb_off + k];
  }
  double pv[TU][MMAX], pb[MFMAX];
  int ploc[TU];
#pragma unroll
  for (int u = 0; u < TU; u++) {
    ploc[u] = -1;
#pragma unroll
    for (int i = 0; i < MMAX; i++) pv[u][i] = 0.0;
  }
#pragma unroll
  for (int i = 0; i < MFMAX; i++) pb[i] = 0.0;
  if (fast_pull && ntg > 0) {
#pragma unroll
    for (int u = 0; u < TU; u++)
      if (64 * u < ntg) {
        const int t = lane + 64 * u;
        const int ts = t < ntg ? t : 0;
        const int loc = P.tg_loc[R.tg_beg + ts];
        ploc[u] = t < ntg ? loc : -1;
        const double* src = P.upd + R.ubase + (int64_t)ts * R.m;
#pragma unroll
        for (int i = 0; i < MMAX; i++)
          if (i < R.m) pv[u][i] = src[i];
      }
  }
  if (fast_pull && rhs && R.mf > 0) {
    const double* src = P.updb + R.fbase + (is_row ? lane : 0) * R.mf;
#pragma unroll
    for (int i = 0; i < MFMAX; i++)
      if (i < R.mf) {
        const double v = src[i];
        pb[i] = is_row ? v : 0.0;
      }
  }
  CXK_STAMP(1);
  if (ntg > 0) {
    // descendants published Schur updates: apply them in the reference's order through an LDS
    // copy laid out like the slab ([diag ns x ns | off ns x s]); tg_loc indexes that copy
    const unsigned l0 = is_row ? (unsigned)lane : (unsigned)(ns * ns + (is_sep ? sc : 0) * ns);
#pragma unroll
    for (int j = 0; j < NSMAX; j++)
      if ((is_row || is_sep) && j < ns) my[l0 + j * st] = a[j];
    WaveSync();
    if (fast_pull) {
#pragma unroll
      for (int u = 0; u < TU; u++)
        if (ploc[u] >= 0) {
          double acc = my[ploc[u]];
#pragma unroll
          for (int i = 0; i < MMAX; i++) acc -= pv[u][i];  // unused slots hold 0.0: exact no-ops
          my[ploc[u]] = acc;
        }
    } else {
      for (int t = R.tg_beg + lane; t < R.tg_end; t += 64) {
        const int loc = P.tg_loc[t];
        double acc = my[loc];
        const int q1 = P.tr_ptr[t + 1];
#pragma unroll 4
        for (int q = P.tr_ptr[t]; q < q1; q++) acc -= P.upd[P.tr_src[q]];
        my[loc] = acc;
      }
    }
    WaveSync();
#pragma unroll
    for (int j = 0; j < NSMAX; j++)
      if (j < lim) a[j] = my[l0 + j * st];
  }
  if (fast_pull) {
#pragma unroll
    for (int i = 0; i < MFMAX; i++) a[RB] -= pb[i];
  } else if (rhs && is_row) {
    double acc = a[RB];
    const int q1 = P.fs_ptr[R.start + lane + 1];
#pragma unroll 4
    for (int q = P.fs_ptr[R.start + lane]; q < q1; q++) acc -= P.updb[P.fs_src[q]];
    a[RB] = acc;
  }
  // padding pivots: unit diagonal
#pragma unroll
  for (int j = 0; j < NSMAX; j++)
    if (j >= ns && lane == j) a[j] = 1.0;
  CXK_STAMP(2);
  bool bad = false;
  ElimSteps<NSMAX, SMAX, 0>::run(a, lane, bad, ns);
  CXK_STAMP(3);
  if (bad) {
    if (lane == 0) atomicExch(fail, 1);
    return;
  }
#pragma unroll
  for (int j = 0; j < NSMAX; j++)
    if (j < lim) base[o0 + j * st] = a[j];
  if (rhs && is_row) rhs[R.start + lane] = a[RB];
  CXK_STAMP(4);
  if (is_sep) {
    // U[k][c], k <= c (child-side numbering t = k*s - k(k-1)/2 + (c - k), the reference's S_S
    // enumeration), written straight into the consumer's slot
#pragma unroll
    for (int c = 0; c < SMAX; c++)
      if (c >= sc && c < s) P.upd[pdst[c]] = -a[NSMAX + c];
    if (rhs) P.updb[pdstb] = -a[RB];
  }
  CXK_STAMP(5);
}

// The same step with a STRAIGHT-LINE load phase, for supernodes whose pulls fit the dense slots
// (FastPull): a lone wavefront pays a full memory round trip (~1.2 us, nothing else to switch to)
// for every wait it meets, and the compiler waits for ALL outstanding loads wherever a loaded
// value is consumed inside or behind a branch that itself holds loads.  FactorSupernodeRows'
// branch ladders (per-lane predicates, "if (i < m)") cost it three round trips in a row: panel,
// pulled Schur values, pulled forward values.  Here every load -- panel, right-hand side, publish
// destinations, pull locations, pulled values -- is unconditional with a clamped, always valid
// address (the host pads the tables, kPullPad), nothing is consumed before the last one is
// issued, and unused values are masked afterwards: ONE round trip.  The pull is applied through
// an LDS image laid out like the registers (my[64 j + lane], P.tg_reg), written and read back
// without predicates.  Arithmetic and its order are those of FactorSupernodeRows (masked slots
// subtract 0.0: exact), so both give the same bits.
__device__ __forceinline__ bool FastPull(const SnRec& R) {
  return R.tg_end - R.tg_beg <= kFastTargets && R.m <= kFastSlots && R.mf <= kFastSlots;
}

template <int NSMAX, int SMAX, bool RHS, bool ASM = false, bool ROOTBACK = false>
__device__ __forceinline__ void FactorSupernodeLean(const FactorPlan& P, const SnRec& R,
                                                    double* __restrict__ slab, double* __restrict__ rhs,
                                                    int* __restrict__ fail, double* __restrict__ my,
                                                    const AsmIn* ai = nullptr, int aw2 = 0) {
  static_assert(NSMAX + SMAX <= 64, "one lane per panel row");
  constexpr int RB = NSMAX + SMAX, MMAX = kFastSlots, MFMAX = kFastSlots;
  const int lane = threadIdx.x & 63;
  const int ns = R.ns, s = R.nsep;
  const bool is_row = lane < ns;
  const int sc = lane - NSMAX;
  const bool is_sep = sc >= 0 && sc < s;
  double* base = slab + R.diag_off;
  const unsigned rel = (unsigned)(R.offd_off - R.diag_off);
  const unsigned o0 = is_row ? (unsigned)lane : (is_sep ? rel + (unsigned)(sc * ns) : 0u);
  const unsigned st = is_row ? (unsigned)ns : 1u;
  const int lim = is_row ? lane + 1 : (is_sep ? ns : 0);  // valid j < lim
  CXK_STAMP(0);
  // ---- load phase: no consumer before the last load
  double a[NSMAX + SMAX + 1];
  double rb = 0.0, awv = 0.0, aqv = 0.0;
  if constexpr (ASM) {
    // aw2 = this lane's word of the AsmRec (loaded beside the SnRec): block offsets, then the
    // positions, one byte per panel row
    auto f = [&](int i) { return __builtin_amdgcn_readlane(aw2, i); };
    const double* Gk = ai->G + (((int64_t)f(1) << 32) | (uint32_t)f(0));
    const int64_t roff = ((int64_t)f(3) << 32) | (uint32_t)f(2);
    const int M = f(4);
    const int q = is_row ? lane : (is_sep ? ns + sc : 0);
    const int myp = (__builtin_amdgcn_ds_bpermute(4 * (6 + (q >> 2)), aw2) >> (8 * (q & 3))) & 255;
#pragma unroll
    for (int j = 0; j < NSMAX; j++) {
      const int pj = (f(6 + (j >> 2)) >> (8 * (j & 3))) & 255;  // wave-uniform
      const int hi = myp > pj ? myp : pj, lo = myp > pj ? pj : myp;
      a[j] = Gk[(j < lim) ? hi + lo * M : 0];
    }
    const int pr = is_row ? myp : (f(6) & 255);
    awv = ai->AWc[roff + pr];
    aqv = ai->AQcc[roff + pr];
    if constexpr (RHS) rb = ai->b[R.start + (is_row ? lane : 0)];
  } else {
#pragma unroll
    for (int j = 0; j < NSMAX; j++) a[j] = base[(j < lim) ? o0 + j * st : 0u];
    if constexpr (RHS) rb = rhs[R.start + (is_row ? lane : 0)];
  }
  int pdst[SMAX > 0 ? SMAX : 1], pdstb = 0;
  pdst[0] = 0;
  {
    const int k = is_sep ? sc : 0;
    const int* dst = P.pub_dst + R.upd_off + (k * s - k * (k - 1) / 2 - k);
#pragma unroll
    for (int c = 0; c < SMAX; c++) {
      int cc = c < k ? k : (c < s ? c : s - 1);
      cc = cc < 0 ? 0 : cc;
      pdst[c] = dst[cc];
    }
    if constexpr (RHS && SMAX > 0) pdstb = P.pubb_dst[R.updb_off + k];
  }
  const int ntg = R.tg_end - R.tg_beg;
  const int mlast = R.m > 0 ? R.m - 1 : 0, mflast = R.mf > 0 ? R.mf - 1 : 0;
  double pv0[MMAX], pv1[MMAX], pb[MFMAX];
  int ploc0, ploc1 = 0;
  {
    const int ts = lane < ntg ? lane : 0;
    ploc0 = P.tg_reg[R.tg_beg + ts];
    const double* src = P.upd + R.ubase + (int64_t)ts * R.m;
#pragma unroll
    for (int i = 0; i < MMAX; i++) pv0[i] = src[i < R.m ? i : mlast];
  }
#pragma unroll
  for (int i = 0; i < MMAX; i++) pv1[i] = 0.0;
  if (ntg > 64) {  // wave-uniform; loads only
    const int ts = lane + 64 < ntg ? lane + 64 : 0;
    ploc1 = P.tg_reg[R.tg_beg + ts];
    const double* src = P.upd + R.ubase + (int64_t)ts * R.m;
#pragma unroll
    for (int i = 0; i < MMAX; i++) pv1[i] = src[i < R.m ? i : mlast];
  }
  if constexpr (RHS) {
    const double* src = P.updb + R.fbase + (is_row ? lane : 0) * R.mf;
#pragma unroll
    for (int i = 0; i < MFMAX; i++) pb[i] = src[i < R.mf ? i : mflast];
  }
  CXK_STAMP(1);
  // ---- consumers
  if constexpr (ASM) {
    // what assemble_gather would have produced: sums that start from +0.0 (a -0.0 source ends up
    // +0.0), AW / AQc of the own variables for the kernels that follow, and the right-hand side
#pragma unroll
    for (int j = 0; j < NSMAX; j++) a[j] = 0.0 + a[j];
    awv = 0.0 + awv;
    aqv = 0.0 + aqv;
    if (is_row) {
      ai->AW[R.start + lane] = awv;
      ai->AQc[R.start + lane] = aqv;
    }
    if constexpr (RHS) {
      // the expressions of build_rhs / build_rhs_comb, term for term
      if (ai->comb)
        rb = ai->cb * rb + ai->cq * aqv + ai->cw * awv;
      else
        rb = ai->k * (rb * ai->bs + aqv * ai->cs) - 2 * awv;
    }
  }
#pragma unroll
  for (int j = 0; j < NSMAX; j++) a[j] = (j < lim) ? a[j] : 0.0;
#pragma unroll
  for (int c = 0; c < SMAX; c++) a[NSMAX + c] = 0.0;
  a[RB] = (RHS && is_row) ? rb : 0.0;
  if (ntg > 0) {
    // descendants published Schur updates: applied in the reference's order on the LDS image
#pragma unroll
    for (int j = 0; j < NSMAX; j++) my[64 * j + lane] = a[j];
    WaveSync();
    if (lane < ntg) {
      double acc = my[ploc0];
#pragma unroll
      for (int i = 0; i < MMAX; i++) acc -= (i < R.m) ? pv0[i] : 0.0;
      my[ploc0] = acc;
    }
    if (lane + 64 < ntg) {
      double acc = my[ploc1];
#pragma unroll
      for (int i = 0; i < MMAX; i++) acc -= (i < R.m) ? pv1[i] : 0.0;
      my[ploc1] = acc;
    }
    WaveSync();
#pragma unroll
    for (int j = 0; j < NSMAX; j++) a[j] = my[64 * j + lane];
  }
  if constexpr (RHS) {
#pragma unroll
    for (int i = 0; i < MFMAX; i++) a[RB] -= (is_row && i < R.mf) ? pb[i] : 0.0;
  }
  // padding pivots: unit diagonal
#pragma unroll
  for (int j = 0; j < NSMAX; j++)
    if (j >= ns && lane == j) a[j] = 1.0;
  CXK_STAMP(2);
  bool bad = false;
  ElimSteps<NSMAX, SMAX, 0>::run(a, lane, bad, ns);
  CXK_STAMP(3);
  if (bad) {
    if (lane == 0) {
      if constexpr (ASM)
        atomicExch(fail + 1, ai->tag);
      else
        atomicExch(fail, 1);
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < NSMAX; j++)
    if (j < lim) base[o0 + j * st] = a[j];
  if constexpr (ROOTBACK) {
    // the chain's last step: the root is solved backward from these registers (tree_chain_lean)
    static_assert(RHS, "the root is solved backward only with a right-hand side");
    const double yv = RootBackward<NSMAX, true>(a, 0.0, a[RB], ns, my);
    if (is_row) rhs[R.start + lane] = yv;
    return;
  }
  if (RHS && is_row) rhs[R.start + lane] = a[RB];
  CXK_STAMP(4);
  if (is_sep) {
#pragma unroll
    for (int c = 0; c < SMAX; c++)
      if (c >= sc && c < s) P.upd[pdst[c]] = -a[NSMAX + c];
    if constexpr (RHS) P.updb[pdstb] = -a[RB];
  }
  CXK_STAMP(5);
}

// b_j <- L_j^{-T} (b_j - sum_c off_j[:,c] y[sep_j[c]]): lane i owns y_i and column i of L
// (col[k] = L[k][i], k > i) in registers; the solved entry travels by v_readlane.
template <int NSMAX, int SMAX>
__device__ inline void BackwardSupernodeRows(const FactorPlan& P, const SnRec& R,
                                             const double* __restrict__ slab,
                                             double* __restrict__ rhs) {
  const int lane = threadIdx.x & 63;
  const int ns = R.ns;
  const bool active = lane < ns;
  const double* D = slab + R.diag_off + (size_t)(active ? lane : 0) * ns;  // column `lane`
  const double* B = slab + R.offd_off + (active ? lane : 0);
  CXK_STAMPB(1);
  double col[NSMAX];
#pragma unroll
  for (int k = 0; k < NSMAX; k++) col[k] = (active && k > lane && k < ns) ? D[k] : 0.0;
  const double dg = active ? D[lane] : 1.0;
  double acc = active ? rhs[R.start + lane] : 0.0;
  const int cnt = R.bs_end - R.bs_beg;
  if (R.nsep_inline == cnt) {
    // separator rows / columns come with the record: y[sep] and off[:, c] load in the same trip
    constexpr int QN = SMAX < 8 ? SMAX : 8;
    double bv[QN > 0 ? QN : 1], yv[QN > 0 ? QN : 1];
#pragma unroll
    for (int q = 0; q < QN; q++) {
      const bool on = q < cnt;
      const unsigned w = (unsigned)R.sep[q];
      yv[q] = on ? rhs[w & 0x3ffffffu] : 0.0;
      bv[q] = (on && active) ? B[(size_t)(w >> 26) * ns] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < QN; q++) acc -= bv[q] * yv[q];
  } else {
#pragma unroll 4
    for (int q = R.bs_beg; q < R.bs_end; q++) {
      const double yq = rhs[P.bs_row[q]];
      if (active) acc -= B[(size_t)P.bs_c[q] * ns] * yq;
    }
  }
  CXK_STAMPB(2);
  const double dinv = 1.0 / dg;
  CXK_STAMPB(3);
#pragma unroll
  for (int k = NSMAX - 1; k >= 0; k--) {
    if (lane == k) acc *= dinv;
    acc = fma(-col[k], ReadLane(acc, k), acc);  // col[k] is zero for lanes >= k
  }
  CXK_STAMPB(4);
  if (active) rhs[R.start + lane] = acc;
}

template <int NSMAX, int SMAX, bool FRESH, typename Sync>
__device__ __forceinline__ void BackwardSupernodeLeanSync(const SnRec& R, const double* __restrict__ slab,
                                                          double* __restrict__ rhs, Sync sync);  // below

template <int NSMAX, int SMAX>
__device__ __forceinline__ void BackwardSupernodeLean(const SnRec& R, const double* __restrict__ slab,
                                                      double* __restrict__ rhs) {
  BackwardSupernodeLeanSync<NSMAX, SMAX, false>(R, slab, rhs, [] {});
}

__device__ __forceinline__ double RhsValue(const RhsIn& ri, const double* __restrict__ rhs, int p) {
  if (ri.form == 0) return rhs[p];
  const double bp = ri.b[p], aq = ri.AQc[p], aw = ri.AW[p];
  const double kk = (ri.form == 1 && ri.k_from) ? ri.k_from[0] : ri.k;
  return ri.form == 1 ? kk * (bp * ri.bs + aq * ri.cs) - 2 * aw : ri.cb * bp + ri.cq * aq + ri.cw * aw;
}

// ForwardSupernodeWave (b_j <- L_j^{-1} (b_j - pulled forward updates), publish t[c] = off[:,c].b)
// in the row-per-lane register layout with a straight-line load phase: lane r < ns holds row r of
// L, lane NSMAX + c holds column c of the off block.  Operations and their order are those of the
// generic kernel (reciprocal of the diagonal, multiply-then-subtract substitution, fma chain over
// the rows for t[c]), so the results are the same bits.  Needs dense forward slots (R.mf <= 8).
template <int NSMAX, int SMAX, bool ROOTBACK = false>
__device__ __forceinline__ void ForwardSupernodeLean(const FactorPlan& P, const SnRec& R,
                                                     const double* __restrict__ slab,
                                                     double* __restrict__ rhs, const RhsIn& ri,
                                                     double* __restrict__ my = nullptr) {
  constexpr int MFMAX = kFastSlots;
  const int lane = threadIdx.x & 63;
  const int ns = R.ns, s = R.nsep;
  const bool is_row = lane < ns;
  const int sc = lane - NSMAX;
  const bool is_sep = sc >= 0 && sc < s;
  const double* base = slab + R.diag_off;
  const unsigned rel = (unsigned)(R.offd_off - R.diag_off);
  const unsigned o0 = is_row ? (unsigned)lane : (is_sep ? rel + (unsigned)(sc * ns) : 0u);
  const unsigned st = is_row ? (unsigned)ns : 1u;
  const int lim = is_row ? lane : (is_sep ? ns : 0);  // strictly lower part of a row; a whole off column
  // ---- load phase: no consumer before the last load
  double a[NSMAX > 0 ? NSMAX : 1];
#pragma unroll
  for (int j = 0; j < NSMAX; j++) a[j] = base[(j < lim) ? o0 + j * st : 0u];
  double dg = base[is_row ? (unsigned)lane * (unsigned)(ns + 1) : 0u];
  double b = RhsValue(ri, rhs, R.start + (is_row ? lane : 0));
  int pdstb = 0;
  if constexpr (SMAX > 0) pdstb = P.pubb_dst[R.updb_off + (is_sep ? sc : 0)];
  const int mflast = R.mf > 0 ? R.mf - 1 : 0;
  double pb[MFMAX];
  {
    const double* src = P.updb + R.fbase + (is_row ? lane : 0) * R.mf;
#pragma unroll
    for (int i = 0; i < MFMAX; i++) pb[i] = src[i < R.mf ? i : mflast];
  }
  // ---- consumers
#pragma unroll
  for (int j = 0; j < NSMAX; j++) a[j] = (j < lim) ? a[j] : 0.0;
  b = is_row ? b : 0.0;
#pragma unroll
  for (int i = 0; i < MFMAX; i++) b -= (is_row && i < R.mf) ? pb[i] : 0.0;
  const double dinv = is_row ? 1.0 / dg : 0.0;
  double dot = 0.0;
#pragma unroll
  for (int k = 0; k < NSMAX; k++) {
    if (lane == k) b *= dinv;
    const double bk = ReadLane(b, k);  // 0.0 for padding rows k >= ns
    if (is_sep)
      dot = fma(a[k], bk, dot);
    else
      b -= a[k] * bk;  // a[k] is zero for lanes <= k
  }
  if constexpr (ROOTBACK) {  // the chain's last step (no separator): straight back down from these registers
    const double yv = RootBackward<NSMAX, false>(a, dg, b, ns, my);
    if (is_row) rhs[R.start + lane] = yv;
    return;
  }
  if (is_row) rhs[R.start + lane] = b;
  if constexpr (SMAX > 0)
    if (is_sep) P.updb[pdstb] = dot;
}

// BackwardSupernodeRows with a straight-line load phase (see FactorSupernodeLean): column of L,
// off-block entries and the separator values y[sep] all load unconditionally from clamped
// addresses, masks are applied afterwards.  Needs the inline separator list (R.nsep_inline == count).
// `sync` runs between the loads that depend on nothing this launch computes (the supernode's own
// panel and forward-solved values) and the loads of the separator's solution: tree_backward_pair
// passes the workgroup barrier behind which the parent's solution becomes visible.
// FRESH: the separator's solution may have been written by another wavefront of this launch.  Its
// addresses are wave-uniform, so the compiler fetches it with SCALAR loads, and the scalar cache
// is not coherent with vector stores (a line another workgroup pulled in before the parent wrote
// it stays stale): workgroup-scope atomic loads go through the vector path instead.
template <int NSMAX, int SMAX, bool FRESH, typename Sync>
__device__ __forceinline__ void BackwardSupernodeLeanSync(const SnRec& R, const double* __restrict__ slab,
                                                          double* __restrict__ rhs, Sync sync) {
  const int lane = threadIdx.x & 63;
  const int ns = R.ns;
  const bool active = lane < ns;
  const double* D = slab + R.diag_off + (size_t)(active ? lane : 0) * ns;  // column `lane`
  const double* B = slab + R.offd_off + (active ? lane : 0);
  CXK_STAMPB(1);
  double col[NSMAX];
#pragma unroll
  for (int k = 0; k < NSMAX; k++) col[k] = D[(active && k > lane && k < ns) ? k : 0];
  double dg = D[active ? lane : 0];
  double acc = rhs[R.start + (active ? lane : 0)];
  const int cnt = R.bs_end - R.bs_beg;
  constexpr int QN = SMAX < 8 ? SMAX : 8;
  double bv[QN > 0 ? QN : 1], yv[QN > 0 ? QN : 1];
#pragma unroll
  for (int q = 0; q < QN; q++) {
    const unsigned w = q < cnt ? (unsigned)R.sep[q] : 0u;
    // unused slots read the diagonal block instead: a supernode without separator has no off
    // block, and the root's would start at the end of the slab
    const double* src = q < cnt ? B + (size_t)(w >> 26) * ns : D;
    bv[q] = src[0];
  }
  sync();
#pragma unroll
  for (int q = 0; q < QN; q++) {
    const unsigned w = q < cnt ? (unsigned)R.sep[q] : 0u;
    if constexpr (FRESH)
      yv[q] = __hip_atomic_load(rhs + (w & 0x3ffffffu), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else
      yv[q] = rhs[w & 0x3ffffffu];
  }
  // ---- consumers
#pragma unroll
  for (int k = 0; k < NSMAX; k++) col[k] = (active && k > lane && k < ns) ? col[k] : 0.0;
  dg = active ? dg : 1.0;
  acc = active ? acc : 0.0;
#pragma unroll
  for (int q = 0; q < QN; q++) acc -= ((q < cnt && active) ? bv[q] : 0.0) * (q < cnt ? yv[q] : 0.0);
  CXK_STAMPB(2);
  const double dinv = 1.0 / dg;
  CXK_STAMPB(3);
#pragma unroll
  for (int k = NSMAX - 1; k >= 0; k--) {
    if (lane == k) acc *= dinv;
    acc = fma(-col[k], ReadLane(acc, k), acc);  // col[k] is zero for lanes >= k
  }
  CXK_STAMPB(4);
  if (active) rhs[R.start + lane] = acc;
}

// LDS-resident fallback for supernodes that do not fit the register kernels.
__device__ inline void CholSupernodeLds(const FactorPlan& P, int p, double* __restrict__ slab,
                                        double* __restrict__ rhs, int* __restrict__ fail,
                                        double* __restrict__ my) {
  const int lane = threadIdx.x & 63;
  const int ns = __builtin_amdgcn_readfirstlane(P.ns[p]), s = __builtin_amdgcn_readfirstlane(P.nsep[p]);
  double* D = slab + P.diag_off[p];
  double* B = slab + P.offd_off[p];
  double* sD = my;
  double* sB = my + ns * ns;
  double* sb = sB + ns * s;
  StageAndPull(P, p, slab, rhs, my, true);
  const int ncols = s + (rhs ? 1 : 0);
  bool bad = false;
  for (int k = 0; k < ns; k++) {
    const double akk = sD[k + k * ns];
    if (!(akk > 0.0)) {
      bad = true;
      break;
    }
    const double d = sqrt(akk);
    WaveSync();
    for (int i = k + lane; i < ns; i += 64) sD[i + k * ns] = (i == k) ? d : sD[i + k * ns] / d;
    for (int c = lane; c < ncols; c += 64) {
      double* col = (c < s) ? sB + c * ns : sb;
      col[k] /= d;
    }
    WaveSync();
    for (int i = k + 1 + lane; i < ns; i += 64) {
      const double lik = sD[i + k * ns];
      for (int j = k + 1; j <= i; j++) sD[i + j * ns] -= lik * sD[j + k * ns];
      for (int c = 0; c < ncols; c++) {
        double* col = (c < s) ? sB + c * ns : sb;
        col[i] -= lik * col[k];
      }
    }
    WaveSync();
  }
  if (bad) {
    if (lane == 0) atomicExch(fail, 1);
    return;
  }
  for (int q = lane; q < ns * ns; q += 64) {
    const int i = q % ns, j = q / ns;
    if (i >= j) D[q] = sD[q];
  }
  for (int q = lane; q < ns * s; q += 64) B[q] = sB[q];
  if (rhs)
    for (int r = lane; r < ns; r += 64) rhs[P.start[p] + r] = sb[r];
  PublishUpdates(P, p, my, true, rhs != nullptr);
}

// b_p <- L_p^{-1} (b_p - published updates); publishes t[c] = off[:,c].b_p.
// Lane i owns b_i; L stays in LDS; the solved entry travels by v_readlane.
__device__ inline void ForwardSupernodeWave(const FactorPlan& P, int p,
                                            const double* __restrict__ slab,
                                            double* __restrict__ rhs, double* __restrict__ my) {
  const int lane = threadIdx.x & 63;
  const int ns = __builtin_amdgcn_readfirstlane(P.ns[p]), s = __builtin_amdgcn_readfirstlane(P.nsep[p]);
  double* sD = my;
  double* sB = my + ns * ns;
  double* sb = sB + ns * s;
  const double* B = slab + P.offd_off[p];
  StageAndPull(P, p, slab, rhs, my, false);
  for (int q = lane; q < ns * s; q += 64) sB[q] = B[q];
  const bool active = lane < ns;
  double b = active ? sb[lane] : 0.0;
  const double dinv = active ? 1.0 / sD[lane + lane * ns] : 0.0;
#pragma unroll 1
  for (int k = 0; k < ns; k++) {
    if (lane == k) b *= dinv;
    const double bk = ReadLane(b, k);
    const double lik = (active && lane > k) ? sD[lane + k * ns] : 0.0;
    b -= lik * bk;
  }
  if (active) {
    rhs[P.start[p] + lane] = b;
    sb[lane] = b;
  }
  WaveSync();
  PublishUpdates(P, p, my, false, true);
}

__device__ inline void ForwardSupernodeLds(const FactorPlan& P, int p,
                                           const double* __restrict__ slab,
                                           double* __restrict__ rhs, double* __restrict__ my) {
  const int lane = threadIdx.x & 63;
  const int ns = __builtin_amdgcn_readfirstlane(P.ns[p]), s = __builtin_amdgcn_readfirstlane(P.nsep[p]);
  double* sD = my;
  double* sB = my + ns * ns;
  double* sb = sB + ns * s;
  const double* B = slab + P.offd_off[p];
  StageAndPull(P, p, slab, rhs, my, false);
  for (int q = lane; q < ns * s; q += 64) sB[q] = B[q];
  for (int k = 0; k < ns; k++) {
    const double bk = sb[k] / sD[k + k * ns];
    WaveSync();
    if (lane == 0) sb[k] = bk;
    for (int i = k + 1 + lane; i < ns; i += 64) sb[i] -= sD[i + k * ns] * bk;
    WaveSync();
  }
  for (int r = lane; r < ns; r += 64) rhs[P.start[p] + r] = sb[r];
  PublishUpdates(P, p, my, false, true);
}

// b_j <- L_j^{-T} (b_j - sum_c off_j[:,c] y[sep_j[c]]) for ns <= 64; lane i owns y_i.
__device__ inline void BackwardSupernodeWave(const FactorPlan& P, int p,
                                             const double* __restrict__ slab,
                                             double* __restrict__ rhs, double* __restrict__ my) {
  const int lane = threadIdx.x & 63;
  const int ns = __builtin_amdgcn_readfirstlane(P.ns[p]);
  const double* D = slab + P.diag_off[p];
  const double* B = slab + P.offd_off[p];
  double* sD = my;
  const bool active = lane < ns;
  const int st = __builtin_amdgcn_readfirstlane(P.start[p]);
  for (int q = lane; q < ns * ns; q += 64) sD[q] = D[q];
  double acc = active ? rhs[st + lane] : 0.0;
  const int q0 = P.bs_ptr[p], q1 = P.bs_ptr[p + 1];
#pragma unroll 4
  for (int q = q0; q < q1; q++) {
    const double yv = rhs[P.bs_row[q]];
    if (active) acc -= B[lane + (size_t)P.bs_c[q] * ns] * yv;
  }
  WaveSync();
  const double dinv = active ? 1.0 / sD[lane + lane * ns] : 0.0;
#pragma unroll 1
  for (int k = ns - 1; k >= 0; k--) {
    if (lane == k) acc *= dinv;
    const double yk = ReadLane(acc, k);
    const double lki = (lane < k) ? sD[k + lane * ns] : 0.0;  // L[k][lane]
    acc -= lki * yk;
  }
  if (active) rhs[st + lane] = acc;
}

__device__ inline void BackwardSupernodeLds(const FactorPlan& P, int p,
                                            const double* __restrict__ slab,
                                            double* __restrict__ rhs, double* __restrict__ my) {
  const int lane = threadIdx.x & 63;
  const int ns = __builtin_amdgcn_readfirstlane(P.ns[p]);
  const double* D = slab + P.diag_off[p];
  const double* B = slab + P.offd_off[p];
  double* sD = my;
  double* sb = my + ns * ns;
  const int st = __builtin_amdgcn_readfirstlane(P.start[p]);
  for (int q = lane; q < ns * ns; q += 64) sD[q] = D[q];
  for (int r = lane; r < ns; r += 64) {
    double acc = rhs[st + r];
    for (int q = P.bs_ptr[p]; q < P.bs_ptr[p + 1]; q++)
      acc -= B[r + (size_t)P.bs_c[q] * ns] * rhs[P.bs_row[q]];
    sb[r] = acc;
  }
  WaveSync();
  for (int k = ns - 1; k >= 0; k--) {
    const double yk = sb[k] / sD[k + k * ns];
    WaveSync();
    if (lane == 0) sb[k] = yk;
    for (int i = lane; i < k; i += 64) sb[i] -= sD[k + i * ns] * yk;
    WaveSync();
  }
  for (int r = lane; r < ns; r += 64) rhs[st + r] = sb[r];
}

}  // namespace cxk
