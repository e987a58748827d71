// Argument structs of the vector-cone kernels, the constant block, the mailbox and the tail workgroup (plain data, no
// device code: safe to include from several translation units, beside lmi_types.h).  The host header of the per-cone
// units (cone_units.h) and the kernel headers of the families share them.
#pragma once
#include "lmi_types.h"
#include "mu_rule.h"

namespace cxk {

struct VecGroup {  // linear: len = rows ; SOC: len = n + 1
  int len;
  int m;
  int count;
  const double* A;  // count x (len x m), col-major
  const double* c;  // count x len
  double* W;        // count x len   (SOC: W[0] = W0, W[1:] = W1)
  double* T1;       // count x len   linear temp_1 / SOC d (d0, d1)
  double* T2;       // count x len   linear temp_2 (d)
  const int* ids;
};

// PerformLineSearch(LinearConstraint*) + FindMinimumMu (linear_constraint.cc:48-103):
//   d0 = e + w o (A y0 - c k0),  delta = (e + w o (A y1 - c k1)) - d0,
//   per row the interval of t with |d0 + t delta| <= dinfmax; out[2 id] = max lower end,
//   out[2 id + 1] = min upper end (the caller treats lower > upper as failure).
struct LineSearchArgs {
  const double* y0;     // permuted solve of -2 AW
  const double* y1;     // permuted solve of AQc c_s + b b_s - 2 AW
  const int* cl_ptr;
  const int* cl_perm;
  double c0_weight, c1_weight, dinfmax;
  double* out;          // [2 K]
};

// ----------------------------------------------------------- constant block
struct StaticGroup {
  int m;
  int count;
  const double* Gc;    // count x (m x m)
  const double* AQc0;  // count x m constant AQc (equality constraints: [0; b], equality_constraint.cc:14-30)
  const int* ids;
};

// Streamed second-order cones (kernels_soc_stream.hip.h).  soc_stream_slack serves the streamed quadratic cones through
// the same view, and the Gram product of the tiled linear blocks takes the split rule below.
constexpr int kSocStreamRowTile = 256;   // rows of the slack one workgroup forms (one per thread)
constexpr int kSocStreamMinSplitK = 1024;  // the Gram product is split along len only into pieces at least this long

struct SocStreamGroup {
  VecGroup v;    // len, m, count, A, c, W, T1 (d), ids as the staged kernels read them
  double* WA;    // count x (len x m)   Q(s) a_i, column by column
  double* s;     // count x len         w^{1/2}
  double* wc;    // count x len         Q(s) c
  double* ms;    // count x len         minus the slack; TakeStep keeps exp(d) here
  double* dets;  // count               det(s)
  double* Gf;    // count x (m x m)     2 WA^T WA, lower triangle (the GEMM's output)
};

// K splits of the Gram product of `count` cones: enough workgroups to fill the chip, none shorter than
// kSocStreamMinSplitK (below that the ordered reduction of the partials costs more than it hides).
__host__ __device__ inline int SocStreamSplits(int len, int m, long long count) {
  const long long tiles = (long long)((m + 63) / 64) * ((m + 63) / 64) * (count > 0 ? count : 1);
  const long long by_len = len / kSocStreamMinSplitK;
  const long long by_fill = (512 + tiles - 1) / tiles;
  const long long s = by_len < by_fill ? by_len : by_fill;
  return s < 1 ? 1 : (int)s;
}

// What the host reads after a round trip, written into its pinned mailbox by the first wavefront
// of a workgroup: the four reduction outputs, the six step scalars, the factorization flag, the
// sequence number the host spins on and a checksum (MailboxWrite).
struct MailboxArgs {
  const double* red;   // [4]
  const double* scal;  // [6]
  const int* fail;     // [2]: flag, tag of a failed first-level pivot of a fused launch
  int tag;
  double seq;
  double* mb;          // pinned host memory, 16 doubles; nullptr: no mailbox write
  const double* mu;    // [1] inv_sqrt_mu as the device last selected it (MuRuleArgs), slot 13; may be null
};

// The barrier-parameter selection evaluated where its inputs appear (mode 1, the tail workgroup):
// out[0] <- NextInvSqrtMu(u, the reduced eigenvalue bounds), mu_rule.h.
struct MuRuleArgs {
  int on;
  cxk_mu::Update u;
  double* out;
};

// The tail workgroup of a PrepareStep / eigenvalue-query launch (cone_tail.hip.h: PrepareTailBlock).
struct StepTail {
  double* slots;  // nullptr: no tail workgroup in this launch
  double* rearm;  // the other slot set: consumed by the launch before, armed again by this one while it waits
  int K, mode;
  const unsigned char* mask;
  double* red_out;
  int scal, N;    // scal != 0: the step scalars as well
  const double *b, *AQc, *y, *sys_sc;
  double* scal_out;
  // ny > 0: the Newton direction is still the three solutions of the triple factorization (StepArgs::y3).  The
  // constraints' wavefronts combine the entries they need where they read them; ny further workgroups behind this
  // one write all of y out (DirectionBlock), count themselves in y_done, and this workgroup forms its scalars when
  // the count has reached y_target -- long before the constraints' results arrive.
  int ny;
  double* y_out;
  unsigned long long* y_done;
  unsigned long long y_target;
  MailboxArgs mbx;
  MuRuleArgs rule;  // mode 1: the selection of inv_sqrt_mu on the device
};

}  // namespace cxk
