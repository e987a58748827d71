// The kernels of the stage drivers themselves (kkt_cone_launch.hip, the only unit that includes this header): the
// constant Schur block, the sharded step-slot kernels and the fixed-order reduction of the step outputs.
//
// Reference semantics:
//   QuadraticFunction / SupernodalAssemblerStatic      quadratic_cost.cc:46-57
#pragma once
#include "cone_tail.hip.h"
#include "shard_mark.hip.h"

namespace cxk {

// ----------------------------------------------------------- constant block
__global__ void static_schur(StaticGroup g, Arena ar) {
  const int mem = blockIdx.x, id = g.ids[mem], mm = g.m * g.m;
  const double* src = g.Gc + (size_t)mem * mm;
  double* G = ar.G + ar.g_off[id];
  for (int q = threadIdx.x; q < mm; q += blockDim.x) G[q] = src[q];
  for (int q = threadIdx.x; q < g.m; q += blockDim.x) {
    ar.AWc[ar.r_off[id] + q] = 0;
    ar.AQcc[ar.r_off[id] + q] = g.AQc0[(size_t)mem * g.m + q];
  }
  if (threadIdx.x == 0) {
    ar.sc[2 * id] = 0;
    ar.sc[2 * id + 1] = 0;
  }
}

// Sharded contexts: the ranks' partial step results meet in ONE sum all-reduce.  Rank r writes its
// (up to four) values into slot r of a world x 4 buffer and zeros the other slots (step_slots_fill);
// after the sum every rank holds every rank's values and combines them in RANK ORDER
// (step_slots_reduce): min / max / sum as the mode asks, the sums in one fixed order on every rank.
// mode 0: {sum normsqrd, max norminfd}; mode 1: {min lambda_min, max lambda_max, sum frob, sum trace}.
// Slot 4 world is the time-out mark (ShardMark, shard_mark.hip.h): a whole-tree launch of some rank whose wait ran
// out travels with the reduction to every rank.
__global__ void step_slots_fill(int rank, int world, const double* __restrict__ red, double* __restrict__ slots,
                                const int* __restrict__ fail, int tag, const double* host_flag) {
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < 4 * world; q += gridDim.x * blockDim.x)
    slots[q] = (q >> 2) == rank ? red[q & 3] : 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) slots[4 * world] = ShardMark(fail, tag, host_flag);
}
__global__ void step_slots_reduce(int mode, int world, const double* __restrict__ slots, double* __restrict__ red,
                                  int* __restrict__ fail, int tag) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  ShardMarkSeen(slots[4 * world], fail, tag);
  double v0 = slots[0], v1 = slots[1], v2 = slots[2], v3 = slots[3];
  for (int r = 1; r < world; r++) {
    const double* s = slots + 4 * r;
    if (mode == 0) {
      v0 += s[0];
      v1 = fmax(v1, s[1]);
    } else {
      v0 = fmin(v0, s[0]);
      v1 = fmax(v1, s[1]);
      v2 += s[2];
      v3 += s[3];
    }
  }
  red[0] = v0;
  red[1] = v1;
  if (mode != 0) {
    red[2] = v2;
    red[3] = v3;
  }
}

// Fixed-order reduction of the per-constraint step outputs on one workgroup.
// mode 0: info2 -> {sum normsqrd, max norminfd (init -1)}
// mode 1: info4 -> {min lambda_min (init 30000), max lambda_max (init -30000), sum frob, sum trace}
__global__ void __launch_bounds__(256)
reduce_step_info(int K, int mode, const double* __restrict__ info, const unsigned char* __restrict__ mask,
                 double* __restrict__ out, MailboxArgs mbx, MuRuleArgs rule) {
  double a = 0, b = (mode == 0) ? -1.0 : 30000.0, c = -30000.0, d = 0;
  // eight strided constraints per trip, loads issued together (a plain loop pays two dependent
  // round trips -- mask, values -- per element); accumulation order unchanged
  constexpr int U = 8;
  for (int i0 = threadIdx.x; i0 < K; i0 += U * blockDim.x) {
    bool on[U];
    double v[U][4];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int i = i0 + u * blockDim.x;
      const int ic = i < K ? i : 0;
      on[u] = mask[ic] != 0 && i < K;
      if (mode == 0) {
        v[u][0] = info[2 * ic];
        v[u][1] = info[2 * ic + 1];
        v[u][2] = v[u][3] = 0.0;
      } else {
#pragma unroll
        for (int q = 0; q < 4; q++) v[u][q] = info[4 * ic + q];
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      if (!on[u]) continue;
      if (mode == 0) {
        a += v[u][0];
        b = fmax(b, v[u][1]);
      } else {
        b = fmin(b, v[u][0]);
        c = fmax(c, v[u][1]);
        a += v[u][2];
        d += v[u][3];
      }
    }
  }
  ReduceStepFinish(mode, a, b, c, d, out, mbx, nullptr, 0.0, &rule);
}

}  // namespace cxk
