// Sparse-LMI Schur assembly.
//
// The C-ABI builds matrix inequalities entry by entry (CONEX_UpdateLinearOperator,
// hermitian_psd.cc:249-275), so the A_i of real programs hold a handful of nonzeros while the
// reference -- and the dense kernels here -- stream and multiply full n x n matrices.  For a
// constraint whose matrices are sparse enough (see LmiSparsePays) the same quantities
//
//   G(i,j) = tr(W A_i W A_j) = sum_{(r,c,a) in A_i} sum_{(p,q,b) in A_j} a b W[c,p] W[q,r]
//   AW(i)  = tr(A_i W)       = sum_{(r,c,a) in A_i} a W[c,r]
//   AQc(i) = G(i, C),  <c,Qc> = G(C, C),  <w,c> = AW(C)       (C = matrix number m)
//
// (dense_lmi_constraint.cc:72-103, hermitian_psd.cc:171-230) are evaluated from the nonzeros:
// O((sum nnz)^2) instead of O(n^3 m + n^2 m^2), and the m n^2 stream of A disappears from HBM
// (the dense A is never uploaded).  A dense affine term C (more than 64 nonzeros) does not join
// the pair sums: X = W C W is formed densely instead (LDS for small orders, two GEMM launches
// otherwise) and AQc(i) = sum a X[c,r], <c,Qc> = sum C o X, <w,c> = sum C o W.
// Beyond the LDS-resident orders such a C can instead be taken by its nonzeros (cxk_set_sparse_affine; the kernels
// lmi_affine_wc / _x / _scalars below): W C W is then formed only at the positions that an entry of some A_i or of C reads.
// Values equal the dense path's up to summation order (tolerance parity,
// tests/test_gpu_sparse.py); every sum has a fixed order: bit-reproducible.
//
// Entry lists hold BOTH triangles of every matrix (the trace inner products above run over the
// full matrix).  Layout per group, m1 = m + 1 lists per member: entries of (member, i) at
// [eptr[mem*m1+i], eptr[mem*m1+i+1]), erc = row | col << 16, eval = value; list m is C (empty
// when C takes the dense route).  The slack of PrepareStep uses a second, position-major copy
// (kernels_lmi.hip.h / kernels_lmi_large.hip.h: sp_pptr / sp_pvar / sp_pval) so that every
// entry of sum_i y_i A_i is accumulated by one thread in the reference's order of i.
#pragma once
#include <type_traits>

#include "kernels_lmi.hip.h"

namespace cxk {

// The pair sums cost about (sum nnz)^2 / 2 terms; a term is four scattered reads (entry pair, two
// W elements).  Measured term rates on MI355X against the dense kernels' flop rates give the
// break-even ratios below (dense flops per sparse term): ~80 where W sits in LDS and the dense
// side is the fused kernel, ~40 for the other LDS-resident shapes, ~300 beyond LDS (W read from
// L2/HBM, dense side on the MFMA GEMM pipeline at 25-40 TFLOP/s).
inline bool LmiSparsePays(int n, int m, double nnz_a, bool lds_resident, bool fused) {
  const double dense = 4.0 * n * n * n * (m + 1.0) + (double)n * n * m * m;
  const double per_term = lds_resident ? (fused ? 80.0 : 40.0) : 300.0;
  return 0.5 * nnz_a * nnz_a * per_term <= dense;
}

#ifdef CXK_DEBUG_STAMPS
__device__ long long g_sparse_stamp[8];
#define SPSTAMP(i) do { if (blockIdx.x == 500 && blockIdx.y == 0 && threadIdx.x == 0) g_sparse_stamp[i] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define SPSTAMP(i) do { } while (0)
#endif

struct SparseLaunch {
  const double* Xg;    // count x n^2: W C W from the GEMM path (large orders with a dense C), else null
  const double* part;  // count x npart x 2: partial sums of <w,c>, <c,Qc> (lmi_dense_c_scalars)
  int npart;
  int emax;            // entries reserved in LDS per workgroup (STAGE)
  int cdense;          // C takes the dense route
};
// ... of the instances behind the affine term by its nonzeros (AFF; SparseAffine below): W C W at the group's positions,
// member mem's from ppos[mem] on, and the slot there of every entry of the A_i.  The other instances take the plain
// struct: their code is what it was.
struct SparseLaunchAffine : SparseLaunch {
  const double* Xp;
  const int* eslot;
  const int* ppos;
};
// ... of the folded instances (FOLD; "The folded sums" below): etop[mem * (m + 1) + i], the number of entries of list
// (mem, i) that lie in the top block row of the real representation.  They stand first in the list.
template <class Base>
struct SparseLaunchFolded : Base {
  const int* etop;
};
template <bool AFF, bool FOLD = false>
using SparseLaunchOf = typename std::conditional<
    FOLD, SparseLaunchFolded<typename std::conditional<AFF, SparseLaunchAffine, SparseLaunch>::type>,
    typename std::conditional<AFF, SparseLaunchAffine, SparseLaunch>::type>::type;

// Dense C beyond LDS-resident orders: partial sums of <w,c> = sum C o W and <c,Qc> = sum C o X over
// slices of the n^2 positions; grid (npart, count).  The sparse kernel adds them in block order.
__global__ void __launch_bounds__(256) lmi_dense_c_scalars(LmiGroup g, const double* __restrict__ Xg,
                                                           double* __restrict__ part) {
  __shared__ double red[16];
  const int nn = g.n * g.n, mem = blockIdx.y;
  const double* Cm = g.C + (size_t)mem * nn;
  const double* Wg = g.W + (size_t)mem * nn;
  const double* X = Xg + (size_t)mem * nn;
  const int per = (nn + gridDim.x - 1) / gridDim.x;
  const int q0 = per * blockIdx.x, q1 = q0 + per < nn ? q0 + per : nn;
  double wc = 0, cq = 0;
  for (int q = q0 + threadIdx.x; q < q1; q += blockDim.x) {
    const double c = Cm[q];
    wc = fma(c, Wg[q], wc);
    cq = fma(c, X[q], cq);
  }
  wc = BlockSum(wc, red);
  cq = BlockSum(cq, red + 8);
  if (threadIdx.x == 0) {
    part[((size_t)mem * gridDim.x + blockIdx.x) * 2] = wc;
    part[((size_t)mem * gridDim.x + blockIdx.x) * 2 + 1] = cq;
  }
}

// ---- The affine term of a group beyond the LDS-resident orders from C's nonzeros (cxk_set_sparse_affine): instead of
// X = W C W by two n^3 GEMMs and sums over all n^2 positions,
//   U = (W C)':  U[p,c] = sum_{q in column p of C} C[q,p] W[c,q]          (lmi_affine_wc:  n nnz(C) multiply-adds)
//   X[c,r] = sum_p U[p,c] W[p,r]  at the positions (c,r) of P only        (lmi_affine_x:   n |P| multiply-adds)
//   <w,c> = sum_{(q,p) in C} C[q,p] W[p,q],  <c,Qc> = sum C[q,p] X[p,q]   (lmi_affine_scalars, slices as lmi_dense_c_scalars)
//   AQc(i) = sum_{(r,c,a) in A_i} a X[c,r]                                (lmi_schur_sparse, through SparseLaunch::eslot)
// P: the distinct positions that an entry of some A_i or of C names.  W is read as stored: nothing but the symmetry of
// C, which cxk_add_lmi_coo makes and the route demands, is used.  The product is kept transposed so that both W and U
// are read down their columns: lmi_affine_wc reads W with the lanes along a column and turns its 64 x 64 tile in LDS,
// lmi_affine_x multiplies two columns.  Every sum has a fixed order; no atomics.
struct SparseAffine {
  const int* cptr;    // (n + 1) per member: column p of its C is [cptr[p], cptr[p + 1]) of crc / cval / cslot
  const int* crc;     // row | col << 16, rows ascending within a column
  const int* cslot;   // the slot in P of position (col, row)
  const double* cval;
  const int* pptr;    // count + 1: member mem's positions are [pptr[mem], pptr[mem + 1]) of prc and of Xp
  const int* prc;     // r | c << 16 of position (c, r), ascending: a run of positions shares the column c of U
  double* U;          // count x n^2
  double* Xp;
};

// grid (tiles of 64 c, tiles of 64 p, count).  A wavefront takes 16 of the tile's columns p with its lanes along c:
// every load of W is one contiguous run of a column; the bounds and entries of column p are wavefront-uniform.
__global__ void __launch_bounds__(256) lmi_affine_wc(LmiGroup g, SparseAffine a) {
  __shared__ double tile[64 * 65];
  const int n = g.n, mem = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c0 = blockIdx.x * 64, p0 = blockIdx.y * 64, c = c0 + lane;
  const double* W = g.W + (size_t)mem * n * n;
  const int* cp = a.cptr + (size_t)mem * (n + 1);
  for (int pl = wave; pl < 64; pl += 4) {
    const int p = p0 + pl;
    double s = 0;
    if (p < n && c < n) {
      const int e1 = cp[p + 1];
#pragma unroll 4
      for (int e = cp[p]; e < e1; e++) s = fma(a.cval[e], W[c + (size_t)(a.crc[e] & 0xffff) * n], s);
    }
    tile[lane * 65 + pl] = s;
  }
  __syncthreads();
  double* U = a.U + (size_t)mem * n * n;
  const int p = p0 + lane;
  for (int cl = wave; cl < 64; cl += 4)
    if (p < n && c0 + cl < n) U[p + (size_t)(c0 + cl) * n] = tile[cl * 65 + lane];
}

// grid (positions / 4, count): a wavefront per position, its lanes down the two columns, four independent partial
// sums per lane, then the fixed butterfly over the lanes.
__global__ void __launch_bounds__(256) lmi_affine_x(LmiGroup g, SparseAffine a) {
  const int n = g.n, mem = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = a.pptr[mem], k = blockIdx.x * 4 + wave;
  if (k >= a.pptr[mem + 1] - b) return;
  const int rc = a.prc[b + k], r = rc & 0xffff, c = rc >> 16;
  const double* Uc = a.U + (size_t)mem * n * n + (size_t)c * n;
  const double* Wr = g.W + (size_t)mem * n * n + (size_t)r * n;
  double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  int q = lane;
  for (; q + 192 < n; q += 256) {
    s0 = fma(Uc[q], Wr[q], s0);
    s1 = fma(Uc[q + 64], Wr[q + 64], s1);
    s2 = fma(Uc[q + 128], Wr[q + 128], s2);
    s3 = fma(Uc[q + 192], Wr[q + 192], s3);
  }
  for (; q < n; q += 64) s0 = fma(Uc[q], Wr[q], s0);
  double s = (s0 + s1) + (s2 + s3);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if (lane == 0) a.Xp[b + k] = s;
}

// Partial sums of <w,c> and <c,Qc> over slices of C's nonzeros, in the layout of lmi_dense_c_scalars (lmi_schur_sparse
// adds them in block order); grid (npart, count).
__global__ void __launch_bounds__(256) lmi_affine_scalars(LmiGroup g, SparseAffine a, double* __restrict__ part) {
  __shared__ double red[16];
  const int n = g.n, mem = blockIdx.y;
  const double* Wg = g.W + (size_t)mem * n * n;
  const double* Xp = a.Xp + a.pptr[mem];
  const int* cp = a.cptr + (size_t)mem * (n + 1);
  const int b = cp[0], nz = cp[n] - b;
  const int per = (nz + gridDim.x - 1) / gridDim.x;
  const int e0 = b + per * blockIdx.x, e1 = e0 + per < b + nz ? e0 + per : b + nz;
  double wc = 0, cq = 0;
  for (int e = e0 + threadIdx.x; e < e1; e += blockDim.x) {
    const int rc = a.crc[e], row = rc & 0xffff, col = rc >> 16;
    const double v = a.cval[e];
    wc = fma(v, Wg[col + (size_t)row * n], wc);
    cq = fma(v, Xp[a.cslot[e]], cq);
  }
  wc = BlockSum(wc, red);
  cq = BlockSum(cq, red + 8);
  if (threadIdx.x == 0) {
    part[((size_t)mem * gridDim.x + blockIdx.x) * 2] = wc;
    part[((size_t)mem * gridDim.x + blockIdx.x) * 2 + 1] = cq;
  }
}

// A folded group (lmi_schur_sparse, "The folded sums") reads W through its projection onto the real representations:
//   X_p[r,c] = 1/d sum_j sign[p][j] W[(p^j) n0 + r, j n0 + c],   Wp block (p^j, j) = sign[p][j] X_p      (n0 = n / d)
// The W that the step kernels leave is a real representation only up to their rounding, which grows with the
// conditioning of W over an interior-point run.  The unfolded sums average that deviation E over the d block rows: for
// real representations A, B,  tr(A (W + E) B (W + E)) = tr(A (W + PE) B (W + PE)) + O(E^2)  with P this (orthogonal)
// projection, because  tr(E S) = tr(PE S)  for every real representation S.  The folded sums read one block row, and on
// W as stored they would see E itself; on PW they give the unfolded value to second order in E.  For a W that is a
// real representation already (cxk_set_W embeds planes) the projection returns its bits: the averages are of equal
// numbers and 1/d is a power of two.  grid (n0^2 / 256, d, count); a thread per plane entry, d reads and d writes;
// fixed order.  W itself is left as it is: the step kernels of a folded group run as those of any other.
// An LDS-resident group (SMALL) needs no launch for it: lmi_schur_sparse projects while it loads W into LDS
// (FoldProjected, the same operations in the same order).
__device__ __forceinline__ int HcSignOf(int p, int j) {
  constexpr int sg[4][4] = {{1, 1, 1, 1}, {1, -1, -1, 1}, {1, 1, -1, -1}, {1, -1, 1, -1}};  // (kHcSign)
  return sg[p][j];
}
// plane p of PW at (r, c): the average over the d blocks that carry it
__device__ __forceinline__ double FoldPlane(const double* __restrict__ W, int n, int n0, int d, int p, int r, int c) {
  double s = 0;
  for (int j = 0; j < d; j++) s += HcSignOf(p, j) * W[(size_t)((p ^ j) * n0 + r) + (size_t)(j * n0 + c) * n];
  return s * (1.0 / d);
}
// entry (row, col) of PW
__device__ __forceinline__ double FoldProjected(const double* __restrict__ W, int n, int n0, int d, int row, int col) {
  const int k = row / n0, j = col / n0, p = k ^ j;
  return HcSignOf(p, j) * FoldPlane(W, n, n0, d, p, row - k * n0, col - j * n0);
}
__global__ void __launch_bounds__(256) lmi_fold_project(LmiGroup g, double* __restrict__ Wp) {
  const int d = g.herm_d, n = g.n, n0 = n / d, p = blockIdx.y, mem = blockIdx.z;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= n0 * n0) return;
  const int r = q % n0, c = q / n0;
  double* O = Wp + (size_t)mem * n * n;
  const double s = FoldPlane(g.W + (size_t)mem * n * n, n, n0, d, p, r, c);
  for (int j = 0; j < d; j++) O[(size_t)((p ^ j) * n0 + r) + (size_t)(j * n0 + c) * n] = HcSignOf(p, j) * s;
}

// Sum over a group of LPP consecutive lanes (LPP a power of two <= 64) in a fixed butterfly order;
// every lane of the group receives the total.
template <int LPP>
__device__ __forceinline__ double GroupSum(double v) {
  if constexpr (LPP == 4) {  // the same butterfly (xor 2, xor 1) on DPP quad permutations: no LDS crossbar
    v += DppMove<0x4E>(v);   // quad_perm [2,3,0,1]
    v += DppMove<0xB1>(v);   // quad_perm [1,0,3,2]
    return v;
  } else if constexpr (LPP == 2) {
    return v + DppMove<0xB1>(v);
  } else {
#pragma unroll
    for (int d = LPP >> 1; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
  }
}

// Sum of the ni x nj terms  a b W[c,p] W[q,r]  of one pair ((r,c,a) from the first list, (p,q,b)
// from the second) shared by LP consecutive lanes.  The longer list goes across the lanes (lane
// `sub` takes its entries sub, sub + LP, ..), every lane walks the whole shorter list, four entries
// at a time: the lane's own entry fixes a column and a row of W (two base addresses), a term is
// then one packed index, one value, two W elements and three multiply-adds -- ~13 instructions
// where a term-by-term walk over the ni x nj rectangle took ~30 (the kernel is bound by instruction
// issue at the sparse-C4 shape: DESIGN 4.8).  sum_i a_i (sum_j b_j w w): fixed order, bit-reproducible;
// every lane of the group returns the total.
// FOLD: the first list is walked over its top entries only (ti, tj: their counts in the two lists; they stand first),
// the second over all of its entries: after the swap by length, top(longer) x full(shorter).
template <int LP, bool FOLD = false>
__device__ __forceinline__ double PairSum(const int* erc, const double* eval, const double* W, int n, int bi,
                                          int ni, int bj, int nj, int sub, int ti = 0, int tj = 0) {
  if (nj > ni) {  // (uniform over the group)
    int t = bi;
    bi = bj;
    bj = t;
    t = ni;
    ni = nj;
    nj = t;
    if constexpr (FOLD) ti = tj;
  }
  if constexpr (FOLD) ni = ti;
  double s = 0;
  for (int ei = sub; ei < ni; ei += LP) {
    const int rc = erc[bi + ei], r = rc & 0xffff, c = rc >> 16;
    const double a = eval[bi + ei];
    const double* Wc = W + c;                           // W[c + p n]
    const double* Wr = W + __umul24((unsigned)r, (unsigned)n);  // W[q + r n]  (orders < 2^12: 24-bit products, full rate)
    double t = 0;
    int ej = 0;
    for (; ej + 4 <= nj; ej += 4) {
      int pq[4];
      double b[4], w0[4], w1[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        pq[u] = erc[bj + ej + u];
        b[u] = eval[bj + ej + u];
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        w0[u] = Wc[__umul24((unsigned)(pq[u] & 0xffff), (unsigned)n)];
        w1[u] = Wr[pq[u] >> 16];
      }
#pragma unroll
      for (int u = 0; u < 4; u++) t = fma(b[u], w0[u] * w1[u], t);
    }
    for (; ej < nj; ej++) {
      const int pq = erc[bj + ej];
      t = fma(eval[bj + ej], Wc[__umul24((unsigned)(pq & 0xffff), (unsigned)n)] * Wr[pq >> 16], t);
    }
    s = fma(a, t, s);
  }
  return GroupSum<LP>(s);
}

// grid (count, chunks of the pair range).
// SMALL: W (and, for a dense C, X = W C W computed by chunk 0) live in LDS; otherwise W is read
// from HBM/L2.  LPP lanes share the nnz_i x nnz_j terms of one pair (1: a thread per pair, for
// the sparsest lists; 64: a wavefront per pair) -- a term is two dependent LDS hops (entry, then
// the W elements it names), so the terms of a lane are issued four at a time.  STAGE: the
// constraint's entry list is copied to LDS first: a sweep reads entries at unrelated addresses,
// which costs a cache line per lane from L1/L2 but only bank conflicts from LDS.
// AFF (never with SMALL): AQc gathers W C W from the values at the positions.
//
// The folded sums (FOLD: a Hermitian group over C or H, d = herm_d > 1, order n = d n0).  For a real representation
// M = L(X) every diagonal block of M is X_0, so tr M / d is the trace of the top-left n0 x n0 block, and with M a
// product that begins with L(A_i) only the rows r < n0 of L(A_i) reach it:
//   tr(L(A_i) W L(A_j) W) / d = sum_{(r,c,a) in L(A_i), r < n0} sum_{(p,q,b) in L(A_j)} a b W[c,p] W[q,r]
//   tr(L(A_i) X) / d          = sum_{(r,c,a) in L(A_i), r < n0} a X[c,r]            (X = W, or W C W)
// The top block row holds the blocks (0, j) = +-X_j, every plane once: exactly 1 / d of the list.  So every sum over a
// first list runs over its top entries and is multiplied by no 1 / d: d-fold fewer terms.  Within each list the top
// entries stand first (by column, then row), the others behind them (by column, then row); L.etop has the count of
// the former.  A pair (i, j) is top(longer) x full(shorter): the order of summation is fixed by the lists alone.
// <w,c> and <c,Qc> of a dense C (the block sums over n^2 positions) keep the full form and their 1 / d.
// The W (and the W C W) of a folded launch is the projection that lmi_fold_project makes (above).
template <bool SMALL, int LPP, bool STAGE, bool AFF = false, bool FOLD = false>
__global__ void __launch_bounds__(256) lmi_schur_sparse(LmiGroup g, Arena ar, SparseLaunchOf<AFF, FOLD> L) {
  extern __shared__ double lds[];
  const int n = g.n, m = g.m, m1 = m + 1, nn = n * n;
  const int mem = blockIdx.x, id = g.ids[mem];
  const double* Cm = g.C + (size_t)mem * nn;
  const double* Wg = g.W + (size_t)mem * nn;
  const int* gptr = g.sp_eptr + (size_t)mem * m1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const double osc = g.herm_d > 1 ? 1.0 / g.herm_d : 1.0;  // (the sums over n^2 positions of a dense C)
  const double lsc = FOLD ? 1.0 : osc;                      // (the sums over entry lists)
  const bool first = blockIdx.y == 0;
  const bool cdense = L.cdense != 0;
  // LDS: [W | C P X (dense C)] (SMALL), entry values, entry row/col, list pointers
  double* sW = lds;
  double* s_val = lds + (SMALL ? (cdense ? 4 : 1) * (size_t)nn : 0);
  int* s_rc = reinterpret_cast<int*>(s_val + (STAGE ? L.emax : 0));
  int* s_ptr = s_rc + (STAGE ? L.emax : 0);
  int* s_top = reinterpret_cast<int*>(reinterpret_cast<double*>(s_ptr + ((m1 + 3) & ~1)) + 16);  // (FOLD; behind the scratch)
  SPSTAMP(0);
  const int e0 = gptr[0];
  for (int q = threadIdx.x; q <= m1; q += blockDim.x) s_ptr[q] = gptr[q] - (STAGE ? e0 : 0);
  if constexpr (FOLD)
    for (int q = threadIdx.x; q < m1; q += blockDim.x) s_top[q] = L.etop[(size_t)mem * m1 + q];
  const int* erc = g.sp_erc;
  const double* eval = g.sp_eval;
  if (STAGE) {
    const int cnt = gptr[m1] - e0;
    for (int q = threadIdx.x; q < cnt; q += blockDim.x) {
      s_val[q] = g.sp_eval[e0 + q];
      s_rc[q] = g.sp_erc[e0 + q];
    }
    erc = s_rc;
    eval = s_val;
  }
  const double* W = Wg;
  if (SMALL) {
    if constexpr (FOLD) {  // (the projection of lmi_fold_project, made on the way into LDS)
      const int n0 = n / g.herm_d;
      for (int q = threadIdx.x; q < nn; q += blockDim.x) sW[q] = FoldProjected(Wg, n, n0, g.herm_d, q % n, q / n);
    } else {
      for (int q = threadIdx.x; q < nn; q += blockDim.x) sW[q] = Wg[q];
    }
    W = sW;
  }
  __syncthreads();
  SPSTAMP(1);
  // dense C: X = W C W (LDS product here for small orders, GEMM launches before this kernel otherwise)
  const double* X = (cdense && L.Xg) ? L.Xg + (size_t)mem * nn : nullptr;
  const double* Xp = nullptr;  // (AFF: W C W at the positions, and an entry's slot beside the entry in the unstaged list)
  const int* eslot = nullptr;
  if constexpr (AFF) {
    Xp = L.Xp + L.ppos[mem];
    eslot = L.eslot + (STAGE ? e0 : 0);
  }
  if (cdense && SMALL) {
    double* sC = sW + nn;
    double* sP = sC + nn;
    double* sX = sP + nn;
    for (int q = threadIdx.x; q < nn; q += blockDim.x) sC[q] = Cm[q];
    __syncthreads();
    LdsGemm(n, sC, sW, sP);  // C W
    __syncthreads();
    LdsGemm(n, sW, sP, sX);  // W C W
    __syncthreads();
    X = sX;
    if (first) {
      double wc = 0, cq = 0;
      for (int q = threadIdx.x; q < nn; q += blockDim.x) {
        const double c = sC[q];
        wc = fma(c, W[q], wc);
        cq = fma(c, X[q], cq);
      }
      double* red = reinterpret_cast<double*>(s_ptr + ((m1 + 3) & ~1));
      wc = BlockSum(wc, red);
      cq = BlockSum(cq, red + 8);
      if (threadIdx.x == 0) {
        ar.sc[2 * id] = wc * osc;
        ar.sc[2 * id + 1] = cq * osc;
      }
    }
  } else if (cdense && first && threadIdx.x == 0) {
    // <w,c>, <c,Qc>: partial sums of lmi_dense_c_scalars, added in block order
    double wc = 0, cq = 0;
    for (int k = 0; k < L.npart; k++) {
      wc += L.part[((size_t)mem * L.npart + k) * 2];
      cq += L.part[((size_t)mem * L.npart + k) * 2 + 1];
    }
    ar.sc[2 * id] = wc * osc;
    ar.sc[2 * id + 1] = cq * osc;
  }
  {
    // AW(i) = sum a W[c,r] (list m, a sparse C, gives <w,c>) and, for a dense C, AQc(i) = sum a X[c,r]:
    // LPV lanes per list, the lists dealt to all chunks
    const int lists = cdense ? m : m1;
    constexpr int LPV = LPP < 8 ? 8 : LPP;
    const int gpb = blockDim.x / LPV;
    for (int i = blockIdx.y * gpb + threadIdx.x / LPV; i < lists; i += gridDim.y * gpb) {
      double aw = 0, aq = 0;
      int e1 = s_ptr[i + 1];
      if constexpr (FOLD) e1 = s_ptr[i] + s_top[i];
      for (int e = s_ptr[i] + (threadIdx.x % LPV); e < e1; e += LPV) {
        const int rc = erc[e], r = rc & 0xffff, c = rc >> 16;
        const double a = eval[e];
        aw = fma(a, W[c + (size_t)r * n], aw);
        if constexpr (AFF) {
          aq = fma(a, Xp[eslot[e]], aq);
        } else {
          if (cdense) aq = fma(a, X[c + (size_t)r * n], aq);
        }
      }
      aw = GroupSum<LPV>(aw);
      if (cdense) aq = GroupSum<LPV>(aq);
      if (threadIdx.x % LPV == 0) {
        if (i < m) {
          ar.AWc[ar.r_off[id] + i] = aw * lsc;
          if (cdense) ar.AQcc[ar.r_off[id] + i] = aq * lsc;
        } else {
          ar.sc[2 * id] = aw * lsc;
        }
      }
    }
  }
  SPSTAMP(2);
  // pair sums: LPP lanes per pair, the pair range dealt to the chunks; pair t -> (i, j) from the
  // group's table.  Row m (a sparse C: at most 64 nonzeros) rides in the same loop:
  // AQc(j) = G(C, A_j), <c,Qc> = G(C, C).
  double* G = ar.G + ar.g_off[id];
  {
    const long long pairs = cdense ? (long long)m * (m + 1) / 2 : (long long)m1 * (m1 + 1) / 2;
    const long long per = (pairs + gridDim.y - 1) / gridDim.y;
    const long long t0 = per * blockIdx.y, t1 = (t0 + per < pairs) ? t0 + per : pairs;
    const int sub = threadIdx.x % LPP, grp = threadIdx.x / LPP, ngrp = blockDim.x / LPP;
    long long t = t0 + grp;
    int ij_next = t < t1 ? g.sp_pairs[t] : 0;
    for (; t < t1; t += ngrp) {
      const int ij = ij_next, i = ij & 0xffff, j = ij >> 16;
      ij_next = t + ngrp < t1 ? g.sp_pairs[t + ngrp] : 0;  // (asked for a pass ahead: off the chain)
      const int bi = s_ptr[i], bj = s_ptr[j];
      double s;
      if constexpr (FOLD)
        s = PairSum<LPP, true>(erc, eval, W, n, bi, s_ptr[i + 1] - bi, bj, s_ptr[j + 1] - bj, sub, s_top[i], s_top[j]);
      else
        s = PairSum<LPP>(erc, eval, W, n, bi, s_ptr[i + 1] - bi, bj, s_ptr[j + 1] - bj, sub);
      if (sub == 0) {
        if (i < m)
          G[i + (size_t)j * m] = s * lsc;
        else if (j < m)
          ar.AQcc[ar.r_off[id] + j] = s * lsc;
        else
          ar.sc[2 * id + 1] = s * lsc;
      }
    }
  }
#ifdef CXK_DEBUG_STAMPS
  SPSTAMP(3);
  __syncthreads();
  SPSTAMP(4);
#endif
}

// bytes of LDS: matrices, staged entries, list pointers (+ block-reduction scratch), the top counts of a folded group
inline size_t LmiSparseLds(int n, int m, bool small, bool cdense, int emax_staged, bool fold = false) {
  size_t b = small ? sizeof(double) * (cdense ? 4 : 1) * (size_t)n * n : 0;
  b += (size_t)emax_staged * 12;
  b += sizeof(int) * (size_t)((m + 1 + 3) & ~1) + sizeof(double) * 16;
  if (fold) b += sizeof(int) * (size_t)((m + 1 + 1) & ~1);
  return b;
}

}  // namespace cxk
