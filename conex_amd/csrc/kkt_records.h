// Plain record and argument types of the supernodal KKT path: what the host builds (kkt_plans.hip),
// the context keeps (kkt_internal.h) and the kernels read.  Types and constants only -- no device
// function, no kernel (RegisterShape is the one function: the host plans with the shape the device
// dispatches on).  The device code on top: tree_supernode.hip.h (building blocks),
// kernels_tree_level.hip.h, kernels_kkt_vec.hip.h, kernels_kkt_top.hip.h, kernels_kkt_big.hip.h,
// kernels_solve_block.hip.h, tree_fused.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace cxk {

// Assembly gather, one launch:
//   slab[dst[t]] = sum_k G[src[k]], k in [ptr[t], ptr[t+1]) ; src < 0 means structural zero
//   AW/AQc in permuted order (constraint order sums), the two scalars, and -- when with_rhs --
//   y = k (b bs + AQc cs) - 2 AW  (cone_program.cc:409-411).  Also clears the factor flag.
// One record per slab target / per variable: the FIRST source sits in the record, so the common
// entry (one source: everything outside the separator overlaps) costs two dependent memory hops
// (record, value) instead of three (list bounds, list, value); further sources follow in the lists.
struct GatherRec {
  int64_t dst;    // slab offset
  int64_t first;  // index into G, < 0 = structural zero
  int beg, extra; // remaining sources: src[beg .. beg + extra)
};
struct ResidRec {
  int64_t first;  // index into AWc / AQcc, < 0 = none
  int beg, extra;
};

struct GatherArgs {
  int64_t T;
  const GatherRec* rec;
  const int64_t* src;
  const double* G;
  double* slab;
  int N;
  const ResidRec* rrec;
  const int* var_idx;  // residual record t describes variable var_idx[t] (nullptr: variable t)
  const int64_t* rs_src;
  const double* AWc;
  const double* AQcc;
  double* AW;
  double* AQc;
  int K;
  const double* sc;
  double* sys_sc;
  int with_rhs;  // 1: y = k (b bs + AQc cs) - 2 AW (build_rhs), 2: y = cb b + cq AQc + cw AW (build_rhs_comb)
  double k, bs, cs;
  double cb, cq, cw;
  const double* b;
  double* y;
  int* fail;
};

// Everything a wavefront needs to start on one supernode: one 128-byte record per position of
// the level lists (level order), fetched with a single coalesced load.
struct SnRec {
  int p, ns, nsep, start;
  int tg_beg, tg_end;  // pull targets (tg_loc / tr_ptr range)
  int bs_beg, bs_end;  // backward separator list (bs_c / bs_row range)
  int64_t diag_off, offd_off, upd_off;
  int updb_off;
  int m;               // slots per pull target:   upd[ubase + t_local * m + i]
  int64_t ubase;
  int fbase, mf;       // forward-solve slots:     updb[fbase + row * mf + i]
  int nsep_inline;     // > 0: sep[q] = row | column << 26 replaces the bs_* lists
  int pad_[3];
  int sep[8];
};
static_assert(sizeof(SnRec) == 128, "SnRec is read as 32 lanes x 4 bytes");

// A supernode without descendants whose panel is a permuted block of ONE constraint's Schur block
// (the leaves of a clique tree: BuildPlans checks every gather list): the first factor level
// loads it straight from the Schur kernels' output -- G(pos[r], pos[c]) -- together with its
// right-hand side, and the separate assembly launch disappears (the rest of the gather rides in
// the same launch as extra workgroups: tree_factor_level_asm).
struct AsmRec {
  int64_t g_off;          // the constraint's m x m block in G (column-major, lower triangle written)
  int64_t r_off;          // its entries of AWc / AQcc
  int m;
  int pad_;
  unsigned char pos[72];  // panel row q (the ns rows, then the separator rows) -> position in the constraint
};
static_assert(sizeof(AsmRec) == 96, "AsmRec is read as 24 lanes x 4 bytes");
struct AsmIn {
  const AsmRec* rec;  // [level-0 position]
  const double *G, *AWc, *AQcc, *b;
  double *AW, *AQc;
  double k, bs, cs;   // y = k (b bs + AQc cs) - 2 AW  (cone_program.cc:409-411)
  double cb, cq, cw;  // or (comb != 0) y = cb b + cq AQc + cw AW  (cone_program.cc:181, 504)
  int comb;
  int tag;            // a failed pivot writes fail[1] = tag (fail[0] is being reset by the gather beside it)
};

struct FactorPlan {
  const SnRec* rec;          // [level positions]
  // per supernode
  const int* ns;             // [K]
  const int* nsep;           // [K]
  const int* start;          // [K] first permuted index
  const int64_t* diag_off;   // [K]
  const int64_t* offd_off;   // [K]
  // Every supernode publishes its Schur update  U[k,j] = off[:,k].off[:,j] (k <= j, the
  // reference's S_S enumeration) and its forward-solve update t[c] = off[:,c].b  into private
  // slots; ancestors pull single values in increasing child index (the reference's order).
  const int64_t* upd_off;    // [K] offset of the s(s+1)/2 values in `upd`
  const int* updb_off;       // [K] offset of the s values in `updb`
  const int* tg_ptr;         // [K+1] targets of supernode p
  const int* tg_loc;         // local offset inside [diag ns x ns | off ns x s]
  const int* tg_reg;         // the same target in the register-shaped LDS image: 64 * column + lane
  const int* tr_ptr;         // [T+1] contributions of target t
  const int64_t* tr_src;     // index into `upd`
  const int* fs_ptr;         // [N+1] contributions of permuted row r
  const int* fs_src;         // index into `updb`
  // backward: separator columns in the reference's accumulation order
  const int* bs_ptr;         // [K+1]
  const int* bs_c;           // column index c within off block
  const int* bs_row;         // permuted index of separator variable
  double* upd;               // slot-ordered (see BuildPlans)
  double* updb;
  const int* pub_dst;        // [child-side numbering upd_off[p] + t] -> slot in upd
  const int* pubb_dst;       // [updb_off[p] + c] -> slot in updb
};

// Register shape (NSMAX << 8 | SMAX) the factor kernels pick for a supernode of ns columns and s
// separator rows (the dispatch of tree_sweep); 0 = no register kernel.
__host__ __device__ inline int RegisterShape(int ns, int s) {
  if (ns <= 8 && s <= 8) return 8 << 8 | 8;
  if (ns <= 16 && s <= 8) return 16 << 8 | 8;
  if (ns <= 24 && s == 0) return 24 << 8 | 0;
  if (ns <= 24 && s <= 8) return 24 << 8 | 8;
  if (ns <= 32 && s <= 16) return 32 << 8 | 16;
  return 0;
}

constexpr int kPullPad = 64;       // spare elements behind pub_dst / pubb_dst / tg_reg / upd / updb
constexpr int kFastTargets = 128;  // pull targets per supernode (2 per lane)
constexpr int kFastSlots = 8;      // contributions per target / forward contributions per row

// Where a solve-only sweep takes its right-hand side: form 0 from `rhs` (someone built it), form 1 /
// 2 each supernode forms its own rows on the fly -- the expressions of build_rhs / build_rhs_comb,
// term for term -- so that the separate launch that used to fill `rhs` first disappears.
struct RhsIn {
  int form;
  const double *b, *AQc, *AW;
  double k, bs, cs;    // form 1: k (b bs + AQc cs) - 2 AW   (cone_program.cc:409-411)
  double cb, cq, cw;   // form 2: cb b + cq AQc + cw AW      (cone_program.cc:181, 504)
  const double* k_from;  // form 1, not null: k = k_from[0], the barrier parameter the device selected
};

constexpr int kRangeMaxRecs = 96;  // tree_sweep<MODE, true>: records of one workgroup's piece held in LDS (12 KB)
constexpr int kChainRing = 64;     // tree_chain_lean: records of the chain's last steps kept in LDS for the way down

// tree_backward_pair: one workgroup's share of two consecutive levels of the way down
struct BackPairEntry {
  int parent;  // record position of the upper-level supernode, -1: none
  int first;   // record position of the first lower-level supernode of this workgroup
  int count;   // how many (consecutive)
  int pad;
};

// The dense top of the tree (kernels_kkt_top.hip.h: tree_top_dense)
constexpr int kTopMaxSn = 16;
constexpr int kTopMaxCols = 64;

constexpr int kTopMaxImage = 4096;  // doubles: panels of the top, and (aliased) their update slots / the dense matrix
constexpr int kTopRhsSrc = 8;       // external forward-solve sources per top row (fixed width)

struct TopDenseArgs {
  int nt, T;                         // supernodes, total columns
  int ns[kTopMaxSn], nsep[kTopMaxSn], start[kTopMaxSn], row0[kTopMaxSn], base[kTopMaxSn];
  long long diag_off[kTopMaxSn], offd_off[kTopMaxSn];
  // consumer-ordered update slots of supernode k: target t (panel position tg_loc[tg_beg + t])
  // reads upd[ubase + t * m + i], i < m.  Slots fed by supernodes INSIDE the top are never written
  // while this kernel does the top (they stay 0.0 and subtract exactly).
  int ubase[kTopMaxSn], m[kTopMaxSn], tg_beg[kTopMaxSn], ntg[kTopMaxSn], ubase_lds[kTopMaxSn], tg_lds[kTopMaxSn];
  const int* top_off;                // [T*T]: image offset of L(r, j), j <= r, or -1
  const int* rhs_src;                // [T * kTopRhsSrc]: updb slots from below the top feeding row r (padded
                                     // with a slot that is always 0.0)
};

// The exchange kernels of a sharded context (kernels_kkt_vec.hip.h: buffer layout there)
struct ExchangeArgs {
  int64_t n_xs;
  int n_xv;
  const int64_t* xs_off;
  const int* xs_pt;   // exchange entry -> list of this rank's published updates into it (pt_ptr), -1 none
  const int* xv_idx;
  int64_t pt_T;
  const int64_t* pt_dst;
  const int* pt_ptr;
  const int64_t* pt_src;
  const int* pf_ptr;
  const int* pf_src;
  const double* upd;
  const double* updb;
  double* slab;
  double* AW;
  double* AQc;
  const double* b;
  double* y;
  double* sys_sc;
  int* fail;
  int tag;  // a failed pivot in a first level with the assembly folded in is reported as fail[1] == tag
  const double* host_flag;  // pinned word a whole-tree launch's wait that ran out raises (ShardMark)
  double* x;
  double cb, cq, cw;
};

}  // namespace cxk
