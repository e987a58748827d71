// The plain (non-template) kernels of the KKT path that do none of the tree's arithmetic: the
// assembly gather, right-hand sides, step scalars, the vector steps of iterative refinement, the
// exchange kernels of sharded contexts, masked and permuted copies.
// Only kkt_tree_launch.hip includes this header: a plain kernel must be defined in exactly one
// translation unit, and every other unit reaches these through its host functions (kkt_launch.h).
#pragma once
#include "device_utils.h"
#include "kkt_records.h"
#include "shard_mark.hip.h"
#include "tree_supernode.hip.h"  // GatherBody

namespace cxk {

__global__ void __launch_bounds__(256) assemble_gather(GatherArgs a) { GatherBody(a, blockIdx.x, gridDim.x); }

// y = k (b bs + AQc cs) - 2 AW   (cone_program.cc:409-411), all in permuted order
// (reset: when not null, the factorization-failure flag cleared here instead of by a memset launch)
__global__ void build_rhs(int N, double k, double bs, double cs, const double* __restrict__ b,
                          const double* __restrict__ AQc, const double* __restrict__ AW,
                          double* __restrict__ y, int* __restrict__ reset = nullptr,
                          const double* __restrict__ k_from = nullptr) {
  if (reset && blockIdx.x == 0 && threadIdx.x == 0) *reset = 0;
  if (k_from) k = k_from[0];  // the barrier parameter the device selected (cxk_select_mu_async)
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < N; p += gridDim.x * blockDim.x)
    y[p] = k * (b[p] * bs + AQc[p] * cs) - 2 * AW[p];
}

// y = cb b + cq AQc + cw AW : every right-hand side of the IPM loop (cone_program.cc:181, 409-411, 504)
__global__ void build_rhs_comb(int N, double cb, double cq, double cw, const double* __restrict__ b,
                               const double* __restrict__ AQc, const double* __restrict__ AW,
                               double* __restrict__ y, int* __restrict__ reset = nullptr) {
  if (reset && blockIdx.x == 0 && threadIdx.x == 0) *reset = 0;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < N; p += gridDim.x * blockDim.x)
    y[p] = cb * b[p] + cq * AQc[p] + cw * AW[p];
}

// The scalars the host loop needs per iteration (cone_program.cc:343-357, 439-446):
// out = { b.y, AQc.y, |b|^2, |AQc|^2, <w,c>, <c,Qc> } ; one workgroup, fixed summation order.
__global__ void __launch_bounds__(1024)
step_scalars(int N, const double* __restrict__ b, const double* __restrict__ AQc,
             const double* __restrict__ y, const double* __restrict__ sys_sc,
             double* __restrict__ out) {
  __shared__ double red[4][16];
  double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  // sixteen strided elements per trip, all loads issued before the first fma: a plain loop is one
  // dependent memory round trip per element (15 in a row at C4; with 16 slots C4 is ONE trip).
  // Same fma order: same bits (out-of-range slots contribute fma(0, 0, s) = s).
  constexpr int U = 16;
  const double sc0 = sys_sc[0], sc1 = sys_sc[1];
  for (int p0 = threadIdx.x; p0 < N; p0 += U * blockDim.x) {
    double vb[U], vq[U], vy[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int p = p0 + u * blockDim.x;
      const bool on = p < N;
      vb[u] = on ? b[p] : 0.0;
      vq[u] = on ? AQc[p] : 0.0;
      vy[u] = on ? y[p] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      s0 = fma(vb[u], vy[u], s0);
      s1 = fma(vq[u], vy[u], s1);
      s2 = fma(vb[u], vb[u], s2);
      s3 = fma(vq[u], vq[u], s3);
    }
  }
  // four BlockSums (wave sum, then the wave totals added in wave order) behind ONE barrier pair
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  s0 = WaveSum(s0);
  s1 = WaveSum(s1);
  s2 = WaveSum(s2);
  s3 = WaveSum(s3);
  if (lane == 0) {
    red[0][wave] = s0;
    red[1][wave] = s1;
    red[2][wave] = s2;
    red[3][wave] = s3;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    double t = 0;
    for (int w = 0; w < nw; w++) t += red[threadIdx.x][w];
    out[threadIdx.x] = t;
  }
  if (threadIdx.x == 4) out[4] = sc0;
  if (threadIdx.x == 5) out[5] = sc1;
}

// y = AQc cs - b bs  (ComputeMuFromDivergence cone_program.cc:181)
__global__ void build_mu_rhs(int N, double bs, double cs, const double* __restrict__ b,
                             const double* __restrict__ AQc, double* __restrict__ y) {
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < N; p += gridDim.x * blockDim.x)
    y[p] = AQc[p] * cs - b[p] * bs;
}

// Iterative refinement (kkt_matvec, kernels_tree_level.hip.h, forms u and mvb):
//   r = b - K y  gathered per row in list order; y saved and r put in its place.
__global__ void refine_residual(int N, const double* __restrict__ rhs0, const double* __restrict__ u,
                                const int* __restrict__ fs_ptr, const int* __restrict__ fs_src,
                                const double* __restrict__ mvb, double* __restrict__ y,
                                double* __restrict__ ysave) {
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < N; p += gridDim.x * blockDim.x) {
    double ky = u[p];
    for (int q = fs_ptr[p]; q < fs_ptr[p + 1]; q++) ky += mvb[fs_src[q]];
    ysave[p] = y[p];
    y[p] = rhs0[p] - ky;
  }
}

__global__ void refine_add(int N, const double* __restrict__ ysave, double* __restrict__ y) {
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < N; p += gridDim.x * blockDim.x) y[p] = ysave[p] + y[p];
}

// ---------------------------------------------------------------------------------------
// Multi-GPU exchange.  Buffer layout, all doubles:
//   [ T slab entries (n_xs) | AW_T (n_xv) | AQc_T (n_xv) | fwd_T (n_xv) | <w,c> | <c,Qc> | fail | pad ]
// pack:   fold this rank's subtree updates into its PARTIAL top blocks (pre-reduce pulls), then
//         copy the partial top, the partial residuals of top variables and the forward-solve
//         contributions of this rank's subtrees into the buffer.
// unpack: after the caller's sum all-reduce the buffer holds the complete assembled-and-updated
//         top; write it back, rebuild the right-hand side of top variables and latch `fail`.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) exchange_pack(ExchangeArgs a) {
  const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  // slab entries: partial assembled value minus the Schur updates of this rank's subtrees (summed
  // in slot order, then subtracted: what a separate fold launch used to leave in the slab)
  for (int64_t i = gid; i < a.n_xs; i += stride) {
    double v = a.slab[a.xs_off[i]];
    const int t = a.xs_pt[i];
    if (t >= 0) {
      double s = 0;
      for (int q = a.pt_ptr[t]; q < a.pt_ptr[t + 1]; q++) s += a.upd[a.pt_src[q]];
      v -= s;
    }
    a.x[i] = v;
  }
  for (int64_t j = gid; j < a.n_xv; j += stride) {
    const int p = a.xv_idx[j];
    a.x[a.n_xs + j] = a.AW[p];
    a.x[a.n_xs + a.n_xv + j] = a.AQc[p];
    double f = 0;
    for (int q = a.pf_ptr[j]; q < a.pf_ptr[j + 1]; q++) f += a.updb[a.pf_src[q]];
    a.x[a.n_xs + 2 * (int64_t)a.n_xv + j] = f;
  }
  if (gid == 0) {
    const int64_t o = a.n_xs + 3 * (int64_t)a.n_xv;
    a.x[o] = a.sys_sc[0];
    a.x[o + 1] = a.sys_sc[1];
    // both forms of a failed pivot travel: fail[0] (level kernels) and the tagged word of the
    // fused first level -- otherwise only the failing rank would know and the ranks would part ways
    a.x[o + 2] = (a.fail[0] != 0 || (a.tag != 0 && a.fail[1] == a.tag)) ? 1.0 : 0.0;
    a.x[o + 3] = 0;
  }
}

__global__ void __launch_bounds__(256) exchange_unpack(ExchangeArgs a) {
  const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = gid; i < a.n_xs; i += stride) a.slab[a.xs_off[i]] = a.x[i];
  for (int64_t j = gid; j < a.n_xv; j += stride) {
    const int p = a.xv_idx[j];
    const double aw = a.x[a.n_xs + j], aq = a.x[a.n_xs + a.n_xv + j];
    a.AW[p] = aw;
    a.AQc[p] = aq;
    a.y[p] = a.cb * a.b[p] + a.cq * aq + a.cw * aw - a.x[a.n_xs + 2 * (int64_t)a.n_xv + j];
  }
  if (gid == 0) {
    const int64_t o = a.n_xs + 3 * (int64_t)a.n_xv;
    a.sys_sc[0] = a.x[o];
    a.sys_sc[1] = a.x[o + 1];
    if (a.x[o + 2] > 0.0) *a.fail = 1;
  }
}

// Solve-only exchange (right-hand sides after the factorization: mu selection, line search,
// cxk_solve_inplace): only the forward-solve contributions of this rank's subtrees to the top
// variables travel, x[j] = sum of its published t values; after the sum all-reduce every rank
// subtracts the total from its (replicated, complete) right-hand side of the top.
__global__ void __launch_bounds__(256) exchange_pack_solve(ExchangeArgs a) {
  if (blockIdx.x == 0 && threadIdx.x == 0) a.x[a.n_xv] = ShardMark(a.fail, a.tag, a.host_flag);
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < a.n_xv; j += (int64_t)gridDim.x * blockDim.x) {
    double f = 0;
    for (int q = a.pf_ptr[j]; q < a.pf_ptr[j + 1]; q++) f += a.updb[a.pf_src[q]];
    a.x[j] = f;
  }
}
__global__ void __launch_bounds__(256) exchange_unpack_solve(ExchangeArgs a) {
  if (blockIdx.x == 0 && threadIdx.x == 0) ShardMarkSeen(a.x[a.n_xv], a.fail, a.tag);
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < a.n_xv; j += (int64_t)gridDim.x * blockDim.x)
    a.y[a.xv_idx[j]] -= a.x[j];
}
// Factor-only exchange (cxk_factor_async on a sharded context): the forward slots hold nothing
// meaningful, the right-hand side of the top is left alone.
__global__ void __launch_bounds__(256) exchange_unpack_matrix(ExchangeArgs a) {
  const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = gid; i < a.n_xs; i += stride) a.slab[a.xs_off[i]] = a.x[i];
  for (int64_t j = gid; j < a.n_xv; j += stride) {
    const int p = a.xv_idx[j];
    a.AW[p] = a.x[a.n_xs + j];
    a.AQc[p] = a.x[a.n_xs + a.n_xv + j];
  }
  if (gid == 0) {
    const int64_t o = a.n_xs + 3 * (int64_t)a.n_xv;
    a.sys_sc[0] = a.x[o];
    a.sys_sc[1] = a.x[o + 1];
    if (a.x[o + 2] > 0.0) *a.fail = 1;
  }
}

// out[i] = count[i] ? in[i] : 0 -- a rank's share of a vector whose entries are spread over the
// ranks (own subtrees; the replicated top counts on rank 0 only): the sum all-reduce of these
// shares is the whole vector.
__global__ void masked_copy(int n, const unsigned char* __restrict__ count, const double* __restrict__ in,
                            double* __restrict__ out) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = count[i] ? in[i] : 0.0;
}
// per-constraint pairs (2 doubles each) of the constraints this rank owns, zero elsewhere
__global__ void masked_copy_pairs(int K, const unsigned char* __restrict__ owned, const double* __restrict__ in,
                                  double* __restrict__ out) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 2 * K; i += gridDim.x * blockDim.x)
    out[i] = owned[i >> 1] ? in[i] : 0.0;
}

// step_scalars over this rank's share of the variables (see masked_copy); out[4], out[5] are the
// already complete <w,c>, <c,Qc>.  The caller sum-reduces out[0..3] across ranks.
__global__ void __launch_bounds__(1024)
step_scalars_masked(int N, const unsigned char* __restrict__ count, const double* __restrict__ b,
                    const double* __restrict__ AQc, const double* __restrict__ y,
                    const double* __restrict__ sys_sc, double* __restrict__ out) {
  __shared__ double red[16];
  double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  for (int p = threadIdx.x; p < N; p += blockDim.x) {
    if (!count[p]) continue;
    const double vb = b[p], vq = AQc[p], vy = y[p];
    s0 = fma(vb, vy, s0);
    s1 = fma(vq, vy, s1);
    s2 = fma(vb, vb, s2);
    s3 = fma(vq, vq, s3);
  }
  s0 = BlockSum(s0, red);
  s1 = BlockSum(s1, red);
  s2 = BlockSum(s2, red);
  s3 = BlockSum(s3, red);
  if (threadIdx.x == 0) {
    out[0] = s0;
    out[1] = s1;
    out[2] = s2;
    out[3] = s3;
    out[4] = sys_sc[0];
    out[5] = sys_sc[1];
  }
}

// permuted <-> original order copies
__global__ void permute_gather(int N, const int* __restrict__ idx, const double* __restrict__ in,
                               double* __restrict__ out) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x)
    out[i] = in[idx[i]];
}

}  // namespace cxk
