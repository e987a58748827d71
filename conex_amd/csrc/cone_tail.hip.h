// Device functions of the host round trip, no kernel: the mailbox write, the end of the fixed-order reduction of the
// step outputs, and the tail workgroup of a PrepareStep / eigenvalue-query launch.  Their callers are
// reduce_step_info and mailbox_pack (kkt_cone_launch.hip) and lmi_prepare_rows (kernels_lmi_rows.hip.h).
#pragma once
#include "cone_types.h"
#include "device_utils.h"

namespace cxk {

// v: this thread's slot value (threads 0 .. 10 and 13; anything elsewhere).  The twelve values, the sequence
// number the host spins on (slot 11) and a checksum (slot 12) leave in ONE store instruction, no
// fence in between: the host does not rely on the order in which the bytes arrive (they cross PCIe
// as posted writes; with a system-scope fence between data and sequence number -- 2 us per round
// trip -- the sequence number was still seen ahead of the data about once in a thousand round trips
// on a cold box).  It accepts a mailbox only when slot 12 equals the XOR of the sequence number's
// bit pattern and the twelve values', each rotated by its own amount (kMailboxRot: stale slots
// cannot cancel each other the way equal changes of two slots would under a plain XOR).
__host__ __device__ constexpr int MailboxRot(int slot) { return (7 * slot + 1) & 63; }
__device__ __forceinline__ void MailboxWrite(const MailboxArgs& m, double v) {
  const int t = threadIdx.x;
  if (t >= 64) return;
  unsigned long long x = 0ull;
  if (t <= 10 || t == 13) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
    const int r = MailboxRot(t);
    x = r ? (bits << r) | (bits >> (64 - r)) : bits;
  }
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) x ^= (unsigned long long)__shfl_xor((long long)x, d, 64);
  double out = v;
  if (t == 11) out = m.seq;
  if (t == 12) out = __longlong_as_double((long long)(x ^ (unsigned long long)__double_as_longlong(m.seq)));
  if (t <= 13) __hip_atomic_store(m.mb + t, out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// fail[1] == tag: a pivot failed in the first factor level of the latest fused launch
__device__ __forceinline__ double MailboxFailValue(const MailboxArgs& m) {
  return (m.fail[0] != 0 || (m.tag != 0 && m.fail[1] == m.tag)) ? 1.0 : 0.0;
}
__device__ __forceinline__ void MailboxPack(const MailboxArgs& m) {
  const int t = threadIdx.x;
  double v = 0.0;
  if (t < 4) v = m.red[t];
  if (t >= 4 && t < 10) v = m.scal[t - 4];
  if (t == 10) v = MailboxFailValue(m);
  if (t == 13 && m.mu) v = *m.mu;
  MailboxWrite(m, v);
}

// The end of the fixed-order reduction below: the 256 threads' partial results -> out[], and with a
// mailbox the results travel to the host from here (no separate mailbox_pack).
// LOCAL (the tail workgroup): the mailbox takes the reduced values from LDS, the step scalars from
// `scal_lds` (this workgroup formed them) or, like the failure flag, from `pre_value` (threads 4 .. 10:
// their slot's value, read before the wait) -- no memory round trip between the last result and the
// host write.
template <bool LOCAL = false>
__device__ __forceinline__ void ReduceStepFinish(int mode, double a, double b, double c, double d,
                                                 double* __restrict__ out, const MailboxArgs& mbx,
                                                 const double* scal_lds = nullptr, double pre_value = 0.0,
                                                 const MuRuleArgs* rule = nullptr) {
  __shared__ double red[8], red2[8], red3[8], red4[8], res[5];
  // the two BlockSums (wave sum, wave totals added in wave order) and the max / min reductions
  // behind ONE barrier
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (int)(blockDim.x >> 6);
  a = WaveSum(a);
  d = WaveSum(d);
  const double bm = (mode == 0) ? WaveMax(b) : -WaveMax(-b);
  const double cm = WaveMax(c);
  if (lane == 0) {
    red[wave] = bm;
    red2[wave] = cm;
    red3[wave] = a;
    red4[wave] = d;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double B = red[0], C = red2[0], A = 0, D = 0;
    for (int w = 1; w < nw; w++) {
      B = (mode == 0) ? fmax(B, red[w]) : fmin(B, red[w]);
      C = fmax(C, red2[w]);
    }
    for (int w = 0; w < nw; w++) {
      A += red3[w];
      D += red4[w];
    }
    if (mode == 0) {
      out[0] = A;
      out[1] = B;
      if (LOCAL) res[0] = A, res[1] = B;
    } else {
      out[0] = B;
      out[1] = C;
      out[2] = A;
      out[3] = D;
      if (LOCAL) res[0] = B, res[1] = C, res[2] = A, res[3] = D;
      if (rule && rule->on) {  // (not LOCAL: the mailbox reads it back from rule->out behind the fence below)
        cxk_mu::Wse e;
        e.lmin = B;
        e.lmax = C;
        e.frob = A;
        e.trace = D;
        const double v = cxk_mu::NextInvSqrtMu(rule->u, e);
        rule->out[0] = v;
        if (LOCAL) res[4] = v;
      }
    }
  }
  if (!mbx.mb) return;
  if (LOCAL) {
    __syncthreads();
    const int t = threadIdx.x;
    double v = 0.0;
    // (the separate launches send out[2], out[3] as the last mode-1 call left them: nobody reads them in mode 0)
    if (t < (mode == 0 ? 2 : 4)) v = res[t];
    if (t >= 4 && t < 10) v = scal_lds ? scal_lds[t - 4] : pre_value;
    if (t == 10) v = pre_value;
    if (t == 13) v = (mode != 0 && rule && rule->on) ? res[4] : pre_value;
    MailboxWrite(mbx, v);
  } else {
    __threadfence();  // out[] is read back below by other threads of this workgroup
    __syncthreads();
    MailboxPack(mbx);
  }
}

// ---------------------------------------------------------------------------------------------
// The tail workgroup of a PrepareStep / eigenvalue-query launch (lmi_prepare_rows: one workgroup
// more than the constraints need): what reduce_step_info and step_scalars do in launches of their
// own behind it.  The constraints' wavefronts hand their results over through `slots` (four doubles
// per constraint, data-as-flag: armed with kTailSentinel, written with write-through stores, polled
// here with sc1 loads -- MI355X_MICROARCH.md's hand-off rules, as in tree_fused); this workgroup
// first forms the step scalars (they need y only), then takes the results as they arrive, reduces
// them in reduce_step_info's order (the same bits) and writes the mailbox.
constexpr unsigned long long kTailSentinel = 0x7FF4C0DEC0DE7A11ull;
constexpr int kTailSpin = 1 << 20;  // polls before the workgroup gives up (NaNs go out: the solve fails loudly)
typedef unsigned int TailU4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void AgentStore(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// step_scalars (kernels_kkt_vec.hip.h, 1024 threads) on 256: thread r plays threads r, r + 256, r + 512,
// r + 768 -- the same fma chains, the same wave sums (wave (r >> 6) + 4 q of the 1024), the sixteen
// wave totals added in the same order: the same bits.
__device__ inline void StepScalarsOn256(int N, const double* __restrict__ b, const double* __restrict__ AQc,
                                        const double* __restrict__ y, const double* __restrict__ sys_sc,
                                        double* __restrict__ out, double* lds_out, bool y_fresh = false) {
  __shared__ double red[4][16];
  double s[4][4];
#pragma unroll
  for (int q = 0; q < 4; q++)
#pragma unroll
    for (int k = 0; k < 4; k++) s[q][k] = 0.0;
  constexpr int U = 4;
  for (int base = 0; base < N; base += 1024 * U) {
    double vb[4][U], vq[4][U], vy[4][U];
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int p = base + 1024 * u + 256 * q + (int)threadIdx.x;
        const bool on = p < N;
        vb[q][u] = on ? b[p] : 0.0;
        vq[q][u] = on ? AQc[p] : 0.0;
        // (y_fresh: written by other workgroups of this launch -- past this XCD's L2)
        vy[q][u] = on ? (y_fresh ? __hip_atomic_load(y + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : y[p]) : 0.0;
      }
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int u = 0; u < U; u++) {
        s[q][0] = fma(vb[q][u], vy[q][u], s[q][0]);
        s[q][1] = fma(vq[q][u], vy[q][u], s[q][1]);
        s[q][2] = fma(vb[q][u], vb[q][u], s[q][2]);
        s[q][3] = fma(vq[q][u], vq[q][u], s[q][3]);
      }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 4; q++)
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const double t = WaveSum(s[q][k]);
      if (lane == 0) red[k][wave + 4 * q] = t;
    }
  __syncthreads();
  if (threadIdx.x < 4) {
    double t = 0;
    for (int w = 0; w < 16; w++) t += red[threadIdx.x][w];
    out[threadIdx.x] = lds_out[threadIdx.x] = t;
  }
  if (threadIdx.x == 4) out[4] = lds_out[4] = sys_sc[0];
  if (threadIdx.x == 5) out[5] = lds_out[5] = sys_sc[1];
}

// One of the ny workgroups that write the Newton direction out (newton_from_three riding in the launch that reads
// it): write-through stores, then -- behind their completion -- one count per workgroup.
__device__ inline void DirectionBlock(const StepTail& T, const StepArgs& sa, int b) {
  const int i = b * 256 + (int)threadIdx.x;
  if (i < T.N) AgentStore(T.y_out + i, YFromThree(sa.y3, sa.y3_stride, sa.y3_k[0], i));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_fetch_add(T.y_done, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ inline void PrepareTailBlock(const StepTail& T) {
  __shared__ double s_scal[6];
  bool y_ok = true;
  if (T.ny > 0) {  // the direction's workgroups first (a few microseconds; nothing else to do before)
    y_ok = false;
    for (int spin = 0; spin < kTailSpin && !y_ok; spin++) {
      y_ok = __hip_atomic_load(T.y_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= T.y_target;
      if (!y_ok) __builtin_amdgcn_s_sleep(8);
    }
    y_ok = __syncthreads_and(y_ok) != 0;
  }
  if (T.scal) {
    StepScalarsOn256(T.N, T.b, T.AQc, T.y, T.sys_sc, T.scal_out, s_scal, T.ny > 0);
    if (!y_ok) {  // (the wait ran out: NaNs go out, the solve fails loudly)
      __syncthreads();
      if (threadIdx.x < 2) T.scal_out[threadIdx.x] = s_scal[threadIdx.x] = __longlong_as_double(0x7FF8000000000000ll);
    }
  }
  const int K = T.K, mode = T.mode, t = threadIdx.x;
  // what the mailbox carries besides this launch's results: final before the launch
  double pre = 0.0;
  if (T.mbx.mb) {
    if (t >= 4 && t < 10 && !T.scal) pre = T.mbx.scal[t - 4];
    if (t == 10) pre = MailboxFailValue(T.mbx);
    if (t == 13 && T.mbx.mu) pre = *T.mbx.mu;
  }
  // (two slot sets, used in turn: the stores that arm a set again are long complete when the launch
  // that uses it next begins, and none of them sits between this launch's last result and its end)
  const double armed = __longlong_as_double((long long)kTailSentinel);
  for (int i = t; i < 4 * K; i += 256) AgentStore(T.rearm + i, armed);
  double a = 0, b = (mode == 0) ? -1.0 : 30000.0, c = -30000.0, d = 0;
  // A polling round is one or two 16-byte sc1 loads per constraint (8-byte loads of the four values
  // one by one made a round of 1000 constraints cost several microseconds of address processing on
  // this one CU -- more than the launch it replaces); offsets past the buffer return zeros without
  // a memory request.
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(T.slots, 0, K * 32, 0x00020000);
  constexpr int U = 4;
  for (int i0 = t; i0 < K; i0 += U * 256) {
    double v[U][4];
    bool on[U];
    int off[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int i = i0 + u * 256;
      on[u] = i < K && T.mask[i < K ? i : 0] != 0;
      off[u] = i < K ? 32 * i : 0x7ffffff0;
    }
    for (int spin = 0; spin < kTailSpin; spin++) {
      bool pending = false;
#pragma unroll
      for (int u = 0; u < U; u++) {
        TailU4 lo = {0u, 0u, 0u, 0u}, hi = {0u, 0u, 0u, 0u};
        lo = __builtin_amdgcn_raw_buffer_load_b128(rs, off[u], 0, 16);  // (aux 16: sc1)
        if (mode != 0) hi = __builtin_amdgcn_raw_buffer_load_b128(rs, off[u] + 16, 0, 16);
        const unsigned long long w0 = ((unsigned long long)lo.y << 32) | lo.x, w1 = ((unsigned long long)lo.w << 32) | lo.z;
        const unsigned long long w2 = ((unsigned long long)hi.y << 32) | hi.x, w3 = ((unsigned long long)hi.w << 32) | hi.z;
        pending = pending || w0 == kTailSentinel || w1 == kTailSentinel || w2 == kTailSentinel || w3 == kTailSentinel;
        v[u][0] = __longlong_as_double((long long)w0);
        v[u][1] = __longlong_as_double((long long)w1);
        v[u][2] = __longlong_as_double((long long)w2);
        v[u][3] = __longlong_as_double((long long)w3);
      }
      if (!pending) break;
      __builtin_amdgcn_s_sleep(2);
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
  ReduceStepFinish<true>(mode, a, b, c, d, T.red_out, T.mbx, T.scal ? s_scal : nullptr, pre, &T.rule);
}

}  // namespace cxk
