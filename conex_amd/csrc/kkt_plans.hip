// Symbolic plans of a context (host code): dependency levels of the elimination tree and the
// partition of a sharded context, then every index table the kernels read -- gather lists, pull
// lists in consumer order, level segments, the chain at the top, paired downward levels, the
// records of the whole-tree launch, the dense top.  Host code only.
#include "kkt_internal.h"
#include "big_chol.h"

namespace cxk_host {

// ---------------------------------------------------------------- tree structure + partition
// Dependency levels of the supernodal elimination tree and (world > 1) the split into a
// replicated top T (all levels >= cut_level) and per-rank subtrees.
void ComputeTreeStructure(cxk_context* ctx) {
  const Layout& L = ctx->lay;
  const int K = ctx->md.K;
  ctx->t_ns.assign(K, 0);
  ctx->t_nsep.assign(K, 0);
  ctx->t_start.assign(K, 0);
  ctx->t_level.assign(K, 0);
  ctx->t_parent.assign(K, -1);
  for (int e = 0; e < K; e++) {
    ctx->t_ns[e] = L.supernode_size[e];
    ctx->t_nsep[e] = (int)L.separators[e].size();
    ctx->t_start[e] = L.supernode_start[e];
    if (ctx->t_nsep[e] > 0) ctx->t_parent[e] = L.var_to_sn[L.separators[e][0]];
  }
  // a supernode sits one level above every supernode that updates it (children have smaller
  // elimination index, so one ascending pass suffices)
  for (int i = 0; i < K; i++) {
    if (ctx->t_ns[i] == 0) continue;
    for (int v : L.separators[i]) {
      const int p = L.var_to_sn[v];
      if (ctx->t_level[p] < ctx->t_level[i] + 1) ctx->t_level[p] = ctx->t_level[i] + 1;
    }
  }
  ctx->nlev = 0;
  for (int e = 0; e < K; e++)
    if (ctx->t_ns[e] > 0) ctx->nlev = std::max(ctx->nlev, ctx->t_level[e] + 1);
}

double ConstraintWork(const ConstraintRec& c) {
  const double n = c.n, m = c.m;
  switch (c.type) {
    case CXK_LMI:
      // (a Hermitian factored record: n = d x order, P = L(F)' Z has d planes)
      if (c.factors.given) return 4 * n * n * c.factors.R + 2 * n * (double)c.factors.R * c.factors.R * std::max(c.herm_d, 1) + 4 * n * n * n;
      return 4 * n * n * n * (m + 1) + n * n * m * m;
    case CXK_LINEAR: return n * m * m;
    case CXK_SOC: return (n + 1) * m * m;
    case CXK_QUAD: return (n + 1) * m * m;
    case CXK_OCT: return 8 * 64 * 8 * n * n * n * (m + 1) + 8 * n * n * m * m;
    default: return m * m;
  }
}

void PartitionTree(cxk_context* ctx) {
  const int K = ctx->md.K, G = ctx->world;
  ctx->sn_top.assign(K, 0);
  ctx->sn_mine.assign(K, 1);
  ctx->owned.assign(K, 1);
  ctx->cut_level = ctx->nlev;
  ctx->var_valid.assign(ctx->md.N, 1);
  ctx->n_xs = 0;
  ctx->n_xv = 0;
  if (G <= 1) return;
  // Choose the cut: the highest level (smallest replicated top, smallest exchange) whose
  // longest-processing-time assignment of subtrees is balanced within 15 % of the ideal;
  // if no level achieves that, the best-balanced one.
  std::vector<int> root_of(K, -1), owner_of_root(K, 0);
  double total = 0;
  for (int e = 0; e < K; e++) total += ConstraintWork(ctx->cons[ctx->md.clique_order[e]]);
  auto try_cut = [&](int cut, std::vector<int>* roots_out, std::vector<int>* root_of_out,
                     std::vector<int>* owner_out) -> double {
    std::vector<int> ro(K, -1);
    std::vector<double> weight(K, 0.0);
    auto is_top = [&](int e) { return ctx->t_ns[e] > 0 && ctx->t_level[e] >= cut; };
    for (int e = K - 1; e >= 0; e--) {  // parents have larger elimination index
      if (is_top(e)) continue;
      const int par = ctx->t_parent[e];
      ro[e] = (par < 0 || is_top(par)) ? e : ro[par];
    }
    double top_work = 0;
    for (int e = 0; e < K; e++) {
      const double w = ConstraintWork(ctx->cons[ctx->md.clique_order[e]]);
      if (is_top(e))
        top_work += w;
      else
        weight[ro[e]] += w;
    }
    std::vector<int> roots;
    for (int e = 0; e < K; e++)
      if (!is_top(e) && ro[e] == e) roots.push_back(e);
    std::stable_sort(roots.begin(), roots.end(), [&](int a, int b) { return weight[a] > weight[b]; });
    std::vector<double> load(G, top_work / G);
    std::vector<int> owner(K, 0);
    for (int r : roots) {  // longest processing time first, ties to the lowest rank
      int best = 0;
      for (int g = 1; g < G; g++)
        if (load[g] < load[best]) best = g;
      owner[r] = best;
      load[best] += weight[r];
    }
    if (roots_out) *roots_out = roots;
    if (root_of_out) *root_of_out = ro;
    if (owner_out) *owner_out = owner;
    return *std::max_element(load.begin(), load.end());
  };
  int cut = ctx->nlev;
  if (ctx->nlev > 1) {
    int best_cut = std::max(ctx->nlev - 1, 1);
    double best_load = -1;
    for (int c = std::max(ctx->nlev - 1, 1); c >= 1; c--) {
      const double mx = try_cut(c, nullptr, nullptr, nullptr);
      if (best_load < 0 || mx < best_load * 0.999) {
        best_load = mx;
        best_cut = c;
      }
      if (mx <= 1.15 * total / G) {
        best_cut = c;
        break;
      }
    }
    cut = best_cut;
  }
  ctx->cut_level = cut;
  std::vector<int> roots;
  try_cut(cut, &roots, &root_of, &owner_of_root);
  for (int e = 0; e < K; e++) ctx->sn_top[e] = ctx->t_ns[e] > 0 && ctx->t_level[e] >= cut;
  int rr = 0;
  for (int e = 0; e < K; e++) {
    const int i = ctx->md.clique_order[e];
    if (ctx->sn_top[e]) {
      ctx->sn_mine[e] = 1;                             // T is factored by every rank
      ctx->owned[i] = (rr++ % G) == ctx->rank;          // its constraints are dealt round-robin
    } else {
      const bool mine = owner_of_root[root_of[e]] == ctx->rank;
      ctx->sn_mine[e] = mine;
      ctx->owned[i] = mine;
    }
  }
  for (int p = 0; p < ctx->md.N; p++) ctx->var_valid[p] = ctx->sn_mine[ctx->lay.var_to_sn[p]];
  for (int e = 0; e < K; e++)
    if (ctx->sn_top[e]) {
      const int64_t n = ctx->t_ns[e];
      ctx->n_xs += n * (n + 1) / 2 + n * ctx->t_nsep[e];
      ctx->n_xv += (int)n;
    }
}

// ---------------------------------------------------------------- plan building
// ---------------------------------------------------------------- plan building
// BuildPlans (at the end of this file) runs the stages below once per context, in order.
namespace {

// The plan-time environment switches, read once when BuildPlans starts.
struct PlanSwitches {
  bool no_big_dataflow = getenv("CXK_NO_BIG_DATAFLOW") != nullptr;
  bool debug_levels = getenv("CXK_DEBUG_LEVELS") != nullptr;
  bool no_lean = getenv("CXK_NO_LEAN") != nullptr;
  bool no_ranges = getenv("CXK_NO_RANGES") != nullptr;
  bool keep_top = getenv("CXK_KEEP_TOP") != nullptr;
  bool no_chain = getenv("CXK_NO_CHAIN") != nullptr;
  bool no_back_pairs = getenv("CXK_NO_BACK_PAIRS") != nullptr;
  bool no_fused_asm = getenv("CXK_NO_FUSED_ASM") != nullptr;
  bool no_fused_shard = getenv("CXK_NO_FUSED_SHARD") != nullptr;
  bool no_fused_tree = getenv("CXK_NO_FUSED_TREE") != nullptr;
  bool no_fused_wide = getenv("CXK_NO_FUSED_WIDE") != nullptr;
  bool fused_split = getenv("CXK_FUSED_SPLIT") != nullptr;
  bool fused_level_order = getenv("CXK_FUSED_LEVEL_ORDER") != nullptr;
  bool fused_padded_frames = getenv("CXK_FUSED_PADDED_FRAMES") != nullptr;
  bool no_fused_sweep = getenv("CXK_NO_FUSED_SWEEP") != nullptr;
  bool no_top_dense = getenv("CXK_NO_TOP_DENSE") != nullptr;
};

// The running verdict on a strategy: check() folds in one condition and keeps the first that
// failed as the reason, which refuse() prints under CXK_DEBUG_LEVELS (not an error: CXK_SUCCESS).
struct Verdict {
  bool ok = true;
  const char* why = nullptr;
  bool check(bool cond, const char* msg) {
    ok = ok && cond;
    if (!ok && !why) why = msg;
    return ok;
  }
  void note(const char* msg) { check(true, msg); }  // behind a loop that updates ok itself
  int refuse(const PlanSwitches& sw, const char* strategy) const {
    if (sw.debug_levels) fprintf(stderr, "%s not taken: %s\n", strategy, why ? why : "(unnamed check)");
    return CXK_SUCCESS;
  }
};

// Lists -> (ptr, src) and one record per list: the first source, the rest at src[beg, beg + extra)
template <typename Rec>
std::vector<Rec> Flatten(const std::vector<std::vector<int64_t>>& lists, std::vector<int>* ptr, std::vector<int64_t>* src) {
  std::vector<Rec> recs(lists.size());
  ptr->assign(lists.size() + 1, 0);
  for (size_t t = 0; t < lists.size(); t++) {
    for (int64_t q : lists[t]) src->push_back(q);
    (*ptr)[t + 1] = (int)src->size();
    const int len = (*ptr)[t + 1] - (*ptr)[t];
    recs[t].first = len > 0 ? (*src)[(*ptr)[t]] : -1;
    recs[t].beg = (*ptr)[t] + 1;
    recs[t].extra = len > 0 ? len - 1 : 0;
  }
  return recs;
}

// the blocks this rank factors (all of them on a single GPU)
bool BlockWanted(const cxk_context* ctx, int e) { return ctx->world <= 1 || ctx->sn_mine[e]; }

// PlanAssemblyGather -> the fused assembly, the fused tree: the record of every slab entry written
struct AsmGather {
  std::vector<int> entry_of;    // slab offset -> record, -1: none
  std::vector<GatherRec> rec;   // first source, further sources src[beg, beg + extra)
  std::vector<int64_t> src;
};

// PlanResidualGather -> the fused assembly, the fused tree
struct ResidGather {
  std::vector<std::vector<int64_t>> per;  // variable -> its sources, in the gather's order
  std::vector<ResidRec> rec;
};

// PlanUpdateSlots -> every later stage that reads the published updates
struct UpdateSlots {
  std::vector<int64_t> upd_off;  // child-side numbering of a supernode's published Schur values
  std::vector<int> updb_off;     // ... and forward values
  // dense slots of supernode p: target t reads upd[ubase[p] + t * m[p] + i], its targets are
  // [tg_ptr[p], tg_ptr[p + 1]); row r reads updb[fbase[p] + r * mf[p] + i]
  std::vector<int64_t> ubase;
  std::vector<int> tg_ptr, m, fbase, mf;
  std::vector<int> pub_dst, pubb_dst;  // publisher -> slot (padded with kPullPad dump slots)
  int64_t slots = 0;                   // Schur-value slots (slot `slots` is the dump slot)
  int slotsb = 0;                      // forward-value slots (likewise)
  std::vector<int64_t> pt_dst;         // slab targets of the pre-contributed updates (sharded)
  std::vector<std::vector<int>> fs;            // variable -> its forward publishers (child-side numbering)
  std::vector<std::vector<int>> pre_fs_slots;  // variable -> its pre-reduce forward slots (sharded)
};

// PlanBackwardOrder -> the level records: per supernode [ptr[e], ptr[e + 1]) separator columns c
// with their rows, ancestors descending, columns ascending within one ancestor
struct BackwardOrder {
  std::vector<int> ptr, c, row;
};

// PlanExchange -> the fused tree: where a top supernode's entries / variables start in the
// exchange (-1: not in the top)
struct ExchangeLayout {
  std::vector<int64_t> xs, xs_base;
  std::vector<int> xv, xv_base;
};

// ---- assembly gather (UpdateBlocks order: elimination index descending).  In sharded mode
// only the blocks this rank factors are written; sources of constraints owned elsewhere are
// dropped, which leaves PARTIAL sums in the top blocks (completed by the exchange).
int PlanAssemblyGather(cxk_context* ctx, AsmGather* ag) {
  const MatrixData& md = ctx->md;
  const Layout& L = ctx->lay;
  std::vector<int>& entry_of = ag->entry_of;
  entry_of.assign(L.slab_size, -1);
  std::vector<int64_t> dst;
  std::vector<std::vector<int64_t>> srcs;
  auto entry = [&](int64_t off) -> std::vector<int64_t>& {
    if (entry_of[off] < 0) {
      entry_of[off] = static_cast<int>(dst.size());
      dst.push_back(off);
      srcs.emplace_back();
    }
    return srcs[entry_of[off]];
  };
  const bool quirks = ctx->reference_identity > 0;
  for (int e = md.K - 1; e >= 0; e--) {
    const int i = md.clique_order[e];
    const int m = ctx->cons[i].m;
    const int64_t base = ctx->g_off[i];
    const bool mine = ctx->owned[i];
    auto coeff = [&](int a, int b) -> int64_t {  // GetCoeff supernodal_assembler.cc:59-70
      if (a < 0 || b < 0 || !mine) return -1;
      return a >= b ? base + (int64_t)b * m + a : base + (int64_t)a * m + b;
    };
    const IntList& r = md.supernodes_pos[e];
    const IntList& s = md.separators_pos[e];
    const int nse = (int)r.size(), nsp = (int)s.size();
    // The reference's direct_update test (BindDiagonalBlock, supernodal_assembler.cc:72-91) passes
    // on a supernode whose positions are -1, 0, .., m-2 (a fill-in variable in front) and then
    // writes G one row/column off and drops the separator terms -- a defect.
    // Reproduced as written by default (reference identity); cxk_set_reference_identity(ctx, 0) /
    // CXK_REFERENCE_QUIRKS=0 scatters every block by position instead.
    bool misplaced = false;
    if (quirks && nse > 0 && m == nse && r[0] != 0) {
      misplaced = true;
      for (int q = 1; q < nse; q++) misplaced = misplaced && r[q] > r[q - 1];
    }
    if (BlockWanted(ctx, e)) {
      for (int j = 0; j < nse; j++)  // SetLowerTri
        for (int i2 = j; i2 < nse; i2++) {
          auto& v = entry(L.diag_off[e] + (int64_t)j * nse + i2);
          v.clear();
          v.push_back(misplaced ? coeff(i2, j) : coeff(r[i2], r[j]));
        }
      if (nse > 0)
        for (int j = 0; j < nsp; j++)  // Set
          for (int i2 = 0; i2 < nse; i2++) {
            auto& v = entry(L.offd_off[e] + (int64_t)j * nse + i2);
            v.clear();
            v.push_back(misplaced ? (int64_t)-1 : coeff(r[i2], s[j]));
          }
    }
    if (misplaced) continue;  // UpdateBlocks returns before Scatter on a direct update
    int cnt = 0;
    for (int j = 0; j < nsp; j++)  // Scatter
      for (int i2 = j; i2 < nsp; i2++) {
        const int64_t off = L.ss_index[e][cnt++];
        const int owner_sn = L.var_to_sn[L.separators[e][j]];
        if (BlockWanted(ctx, owner_sn)) entry(off).push_back(coeff(s[i2], s[j]));
      }
  }
  std::vector<int> as_ptr;
  ag->rec = Flatten<GatherRec>(srcs, &as_ptr, &ag->src);
  for (size_t t = 0; t < dst.size(); t++) ag->rec[t].dst = dst[t];
  ctx->as_T = (int64_t)dst.size();
  CXK_TRY(ctx->as_dst.upload(dst));
  CXK_TRY(ctx->as_ptr.upload(as_ptr));
  CXK_TRY(ctx->as_src.upload(ag->src));
  CXK_TRY(ctx->as_rec.upload(ag->rec));
  return CXK_SUCCESS;
}

// ---- residual gather (constraint order); variables of foreign subtrees are skipped
int PlanResidualGather(cxk_context* ctx, ResidGather* rg) {
  const int N = ctx->md.N;
  std::vector<std::vector<int64_t>>& per = rg->per;
  per.assign(N, {});
  for (int i = 0; i < (int)ctx->cons.size(); i++) {
    if (!ctx->owned[i]) continue;
    for (int q = 0; q < (int)ctx->cliques[i].size(); q++)
      per[ctx->md.permutation[ctx->cliques[i][q]]].push_back(ctx->r_off[i] + q);
  }
  std::vector<int> ptr;
  std::vector<int64_t> src;
  rg->rec = Flatten<ResidRec>(per, &ptr, &src);
  CXK_TRY(ctx->rs_ptr.upload(ptr));
  CXK_TRY(ctx->rs_src.upload(src));
  CXK_TRY(ctx->rs_rec.upload(rg->rec));
  return CXK_SUCCESS;
}

// ---- clique variables in permuted numbering
int PlanCliqueVariables(cxk_context* ctx) {
  std::vector<int> ptr(ctx->cons.size() + 1, 0), perm;
  for (size_t i = 0; i < ctx->cons.size(); i++) {
    for (int v : ctx->cliques[i]) perm.push_back(ctx->md.permutation[v]);
    ptr[i + 1] = (int)perm.size();
  }
  CXK_TRY(ctx->cl_ptr.upload(ptr));
  CXK_TRY(ctx->cl_perm.upload(perm));
  return CXK_SUCCESS;
}

// ---- published-update slots: s(s+1)/2 Schur values and s forward values per supernode
int PlanUpdateSlots(cxk_context* ctx, UpdateSlots* u) {
  const Layout& L = ctx->lay;
  const int K = ctx->md.K, N = ctx->md.N;
  const std::vector<int>& ns = ctx->t_ns;
  const std::vector<int>& nsep = ctx->t_nsep;
  const std::vector<int>& start = ctx->t_start;
  const bool sharded = ctx->world > 1;
  std::vector<int64_t>& upd_off = u->upd_off;
  std::vector<int>& updb_off = u->updb_off;
  upd_off.assign(K, 0);
  updb_off.assign(K, 0);
  int64_t upd_total = 0;
  int updb_total = 0;
  for (int i = 0; i < K; i++) {
    upd_off[i] = upd_total;
    updb_off[i] = updb_total;
    if (ns[i] > 0) {
      upd_total += (int64_t)nsep[i] * (nsep[i] + 1) / 2;
      updb_total += nsep[i];
    }
  }
  // pull lists.  A target inside a subtree only has children of the same subtree.  A target in
  // the top T pulls its T children during the T sweep; the updates of THIS rank's subtrees are
  // folded in before the exchange (pre-reduce lists pt_* / pf_*).
  std::vector<int> tgt_of(L.slab_size, -1);
  std::vector<std::vector<int>> tg_of_sn(K);
  std::vector<int64_t> tg_dst_all;
  std::vector<std::vector<int64_t>> contrib, pre_contrib;
  std::vector<std::vector<int>>& fs = u->fs;
  std::vector<std::vector<int>> pre_fs(N);
  fs.assign(N, {});
  for (int i = 0; i < K; i++) {
    if (ns[i] == 0 || nsep[i] == 0) continue;
    if (sharded && !ctx->sn_mine[i]) continue;  // foreign subtree: its updates arrive by exchange
    const IntList& s = L.separators[i];
    int cnt = 0;
    for (int k = 0; k < nsep[i]; k++) {
      const int p = L.var_to_sn[s[k]];
      const bool pre = sharded && ctx->sn_top[p] && !ctx->sn_top[i];
      for (int j = k; j < nsep[i]; j++) {
        const int64_t off = L.ss_index[i][cnt];
        if (tgt_of[off] < 0) {
          tgt_of[off] = (int)tg_dst_all.size();
          tg_dst_all.push_back(off);
          contrib.emplace_back();
          pre_contrib.emplace_back();
          tg_of_sn[p].push_back(tgt_of[off]);
        }
        (pre ? pre_contrib : contrib)[tgt_of[off]].push_back(upd_off[i] + cnt);
        cnt++;
      }
      (pre ? pre_fs : fs)[s[k]].push_back(updb_off[i] + k);
    }
  }
  // Slots.  A published value is written straight to the place its (single) consumer reads it
  // from: the contributions of target t of supernode p occupy  upd[ubase_p + t_local * m_p + i],
  // i = position in the reference's accumulation order, m_p = longest list of p (unused slots
  // stay 0.0: subtracting them is exact).  The consumer can therefore issue every load as soon
  // as it knows its record -- no index lists on the critical path.  Publishers look their slot up
  // in pub_dst (indexed by the child-side numbering upd_off[i] + t).  Pre-reduce contributions
  // (subtree -> top, sharded runs) get plain list slots after the dense region.
  u->ubase.assign(K, 0);
  u->m.assign(K, 0);
  u->fbase.assign(K, 0);
  u->mf.assign(K, 0);
  std::vector<int>& pub_dst = u->pub_dst;
  std::vector<int>& pubb_dst = u->pubb_dst;
  pub_dst.assign((size_t)upd_total, -1);
  pubb_dst.assign((size_t)updb_total, -1);
  int64_t& slots = u->slots;
  int& slotsb = u->slotsb;
  {
    std::vector<int>& tg_ptr = u->tg_ptr;
    tg_ptr.assign(K + 1, 0);
    std::vector<int> tr_ptr, tg_loc, tg_reg, pt_ptr;
    std::vector<int64_t> tr_src, pt_src;
    std::vector<int64_t>& pt_dst = u->pt_dst;
    tr_ptr.push_back(0);
    pt_ptr.push_back(0);
    for (int p = 0; p < K; p++) {
      size_t m = 0;
      for (int t : tg_of_sn[p]) m = std::max(m, contrib[t].size());
      u->ubase[p] = slots;
      u->m[p] = (int)m;
      int tl = 0;
      for (int t : tg_of_sn[p]) {
        const int64_t off = tg_dst_all[t];
        const int64_t dsz = (int64_t)ns[p] * ns[p];
        if (!contrib[t].empty()) {
          tg_loc.push_back(off >= L.diag_off[p] && off < L.diag_off[p] + dsz
                               ? (int)(off - L.diag_off[p])
                               : (int)(dsz + off - L.offd_off[p]));
          {
            // the same entry in the register-shaped image of FactorSupernodeLean: 64 * column + lane
            const int nsm = RegisterShape(ns[p], nsep[p]) >> 8, loc = tg_loc.back();
            const int col = loc < dsz ? loc / ns[p] : (int)(loc - dsz) % ns[p];
            const int ln = loc < dsz ? loc % ns[p] : nsm + (int)(loc - dsz) / ns[p];
            tg_reg.push_back(nsm > 0 ? 64 * col + ln : 0);
          }
          for (size_t i = 0; i < contrib[t].size(); i++) {
            const int64_t slot = slots + (int64_t)tl * (int64_t)m + (int64_t)i;
            pub_dst[contrib[t][i]] = (int)slot;
            tr_src.push_back(slot);
          }
          tr_ptr.push_back((int)tr_src.size());
          tl++;
        }
      }
      slots += (int64_t)tl * (int64_t)m;
      tg_ptr[p + 1] = (int)tg_loc.size();
    }
    for (int p = 0; p < K; p++)
      for (int t : tg_of_sn[p])
        if (!pre_contrib[t].empty()) {
          pt_dst.push_back(tg_dst_all[t]);
          for (int64_t q : pre_contrib[t]) {
            pub_dst[q] = (int)slots;
            pt_src.push_back(slots++);
          }
          pt_ptr.push_back((int)pt_src.size());
        }
    CXK_DEMAND(slots < (int64_t)INT32_MAX, "published-update slots exceed 32-bit indexing");
    CXK_TRY(ctx->tg_ptr.upload(tg_ptr));
    CXK_TRY(ctx->tg_loc.upload(tg_loc));
    tg_reg.resize(tg_reg.size() + kPullPad, 0);  // FactorSupernodeLean loads unconditionally (clamped)
    CXK_TRY(ctx->tg_reg.upload(tg_reg));
    CXK_TRY(ctx->tr_ptr.upload(tr_ptr));
    CXK_TRY(ctx->tr_src.upload(tr_src));
    CXK_TRY(ctx->pt_dst.upload(pt_dst));
    CXK_TRY(ctx->pt_ptr.upload(pt_ptr));
    CXK_TRY(ctx->pt_src.upload(pt_src));
  }
  u->pre_fs_slots.assign(N, {});
  {
    std::vector<int> fs_ptr(N + 1, 0), fs_src;
    for (int e = 0; e < K; e++) {
      size_t m = 0;
      for (int r = 0; r < ns[e]; r++) m = std::max(m, fs[start[e] + r].size());
      u->fbase[e] = slotsb;
      u->mf[e] = (int)m;
      slotsb += ns[e] * (int)m;
    }
    for (int e = 0; e < K; e++)
      for (int r = 0; r < ns[e]; r++) {
        const int p = start[e] + r;
        for (size_t i = 0; i < fs[p].size(); i++) pubb_dst[fs[p][i]] = u->fbase[e] + r * u->mf[e] + (int)i;
      }
    for (int p = 0; p < N; p++) {
      for (int q : fs[p]) fs_src.push_back(pubb_dst[q]);
      fs_ptr[p + 1] = (int)fs_src.size();
    }
    for (int p = 0; p < N; p++)
      for (int q : pre_fs[p]) {
        pubb_dst[q] = slotsb;
        u->pre_fs_slots[p].push_back(slotsb++);
      }
    CXK_TRY(ctx->fs_ptr.upload(fs_ptr));
    CXK_TRY(ctx->fs_src.upload(fs_src));
  }
  // values nobody on this rank consumes land in one dump slot at the end
  for (int& d : pub_dst)
    if (d < 0) d = (int)slots;
  for (int& d : pubb_dst)
    if (d < 0) d = slotsb;
  CXK_TRY(ctx->upd_off.upload(upd_off));
  CXK_TRY(ctx->updb_off.upload(updb_off));
  pub_dst.resize(pub_dst.size() + kPullPad, (int)slots);  // padding read (never used) by clamped loads
  pubb_dst.resize(pubb_dst.size() + kPullPad, slotsb);
  CXK_TRY(ctx->pub_dst.upload(pub_dst));
  CXK_TRY(ctx->pubb_dst.upload(pubb_dst));
  CXK_TRY(ctx->upd.alloc((size_t)slots + 1 + kPullPad, true));   // unused slots subtract 0.0
  CXK_TRY(ctx->updb.alloc((size_t)slotsb + 2 + kPullPad, true));  // + dump slot + a slot that stays 0.0
  return CXK_SUCCESS;
}

// ---- exchange layout: [T slab entries | AW_T | AQc_T | fwd_T | <w,c> <c,Qc> fail]
int PlanExchange(cxk_context* ctx, const UpdateSlots& u, ExchangeLayout* x) {
  const Layout& L = ctx->lay;
  const int K = ctx->md.K, N = ctx->md.N;
  const std::vector<int>& ns = ctx->t_ns;
  const std::vector<int>& start = ctx->t_start;
  std::vector<int64_t>& xs = x->xs;
  std::vector<int>& xv = x->xv;
  x->xs_base.assign(K, -1);
  x->xv_base.assign(K, -1);
  if (ctx->world <= 1) return CXK_SUCCESS;
  std::vector<int> pf_ptr, pf_src;
  pf_ptr.push_back(0);
  for (int e = 0; e < K; e++) {
    if (!ctx->sn_top[e]) continue;
    x->xs_base[e] = (int64_t)xs.size();
    x->xv_base[e] = (int)xv.size();
    for (int j = 0; j < ns[e]; j++)
      for (int i2 = j; i2 < ns[e]; i2++) xs.push_back(L.diag_off[e] + (int64_t)j * ns[e] + i2);
    for (int64_t q = 0; q < (int64_t)ns[e] * ctx->t_nsep[e]; q++) xs.push_back(L.offd_off[e] + q);
    for (int r = 0; r < ns[e]; r++) {
      const int p = start[e] + r;
      xv.push_back(p);
      for (int q : u.pre_fs_slots[p]) pf_src.push_back(q);
      pf_ptr.push_back((int)pf_src.size());
    }
  }
  CXK_DEMAND(ctx->n_xs == (int64_t)xs.size() && ctx->n_xv == (int)xv.size(),
             "internal error: exchange layout mismatch");
  CXK_TRY(ctx->xs_off.upload(xs));
  {
    // exchange_pack folds this rank's own Schur updates into its partial top entries on the
    // way out: entry i of the exchange -> its list of published values (pt_ptr), or -1
    std::map<int64_t, int> list_of;
    for (size_t t = 0; t < u.pt_dst.size(); t++) list_of[u.pt_dst[t]] = (int)t;
    std::vector<int> xs_pt(xs.size() + 1, -1);
    size_t found = 0;
    for (size_t i = 0; i < xs.size(); i++) {
      auto it = list_of.find(xs[i]);
      if (it != list_of.end()) {
        xs_pt[i] = it->second;
        found++;
      }
    }
    CXK_DEMAND(found == u.pt_dst.size(), "internal error: a pre-contributed update targets an entry outside the exchange");
    CXK_TRY(ctx->xs_pt.upload(xs_pt));
  }
  CXK_TRY(ctx->xv_idx.upload(xv));
  CXK_TRY(ctx->pf_ptr.upload(pf_ptr));
  CXK_TRY(ctx->pf_src.upload(pf_src));
  CXK_TRY(ctx->xbuf.alloc((size_t)ctx->n_xs + 3 * (size_t)ctx->n_xv + 4));
  std::vector<unsigned char> count(N, 0);
  for (int p = 0; p < N; p++) {
    const int e = L.var_to_sn[p];
    count[p] = ctx->sn_top[e] ? (ctx->rank == 0) : (ctx->sn_mine[e] != 0);
  }
  CXK_TRY(ctx->d_count_mask.upload(count));
  CXK_TRY(ctx->shard_tmp.alloc(std::max<size_t>((size_t)N, 2 * ctx->cons.size())));
  return CXK_SUCCESS;
}

// ---- backward accumulation order: ancestors descending, columns ascending within one ancestor
int PlanBackwardOrder(cxk_context* ctx, BackwardOrder* bo) {
  const Layout& L = ctx->lay;
  const int K = ctx->md.K;
  bo->ptr.assign(K + 1, 0);
  for (int j = 0; j < K; j++) {
    if (ctx->t_ns[j] > 0) {
      const IntList& s = L.separators[j];
      int hi = ctx->t_nsep[j];
      while (hi > 0) {
        const int anc = L.var_to_sn[s[hi - 1]];
        int lo = hi - 1;
        while (lo > 0 && L.var_to_sn[s[lo - 1]] == anc) lo--;
        for (int c = lo; c < hi; c++) {
          bo->c.push_back(c);
          bo->row.push_back(s[c]);
        }
        hi = lo;
      }
    }
    bo->ptr[j + 1] = (int)bo->c.size();
  }
  CXK_TRY(ctx->bs_ptr.upload(bo->ptr));
  CXK_TRY(ctx->bs_c.upload(bo->c));
  CXK_TRY(ctx->bs_row.upload(bo->row));
  return CXK_SUCCESS;
}

// ---- level lists: supernodes with at least one column that this rank factors, sorted into
// segments; big supernodes (beyond LDS) at the end of their level; the level-ordered records
int PlanLevels(cxk_context* ctx, const PlanSwitches& sw, const UpdateSlots& u, const BackwardOrder& bo) {
  const Layout& L = ctx->lay;
  const int K = ctx->md.K, N = ctx->md.N;
  const std::vector<int>& ns = ctx->t_ns;
  const std::vector<int>& nsep = ctx->t_nsep;
  const int nlev = ctx->nlev;
  ctx->level_ptr.assign(nlev + 1, 0);
  ctx->level_sn.clear();
  ctx->chol_lds = 8;
  ctx->level_big.assign(nlev, 0);
  ctx->level_nh.assign(nlev, 0);
  size_t big_ws = 0;
  auto panel_bytes = [&](int e) {
    return sizeof(double) * ((size_t)ns[e] * ns[e] + (size_t)ns[e] * nsep[e] + 3 * (size_t)ns[e] + 2);
  };
  // (register shape, dense pulls, inline separator list) of a supernode: see cxk_context::LevelSeg
  auto seg_fast = [&](int e) {
    return u.tg_ptr[e + 1] - u.tg_ptr[e] <= kFastTargets && u.m[e] <= kFastSlots && u.mf[e] <= kFastSlots;
  };
  auto seg_inline = [&](int e) { return bo.ptr[e + 1] - bo.ptr[e] <= 8 && N < (1 << 26); };
  auto seg_key = [&](int e) { return std::make_tuple(RegisterShape(ns[e], nsep[e]), seg_fast(e), seg_inline(e)); };
  for (int l = 0; l < nlev; l++) {
    std::vector<int> huge;
    for (int e = 0; e < K; e++)
      if (ns[e] > 0 && ctx->t_level[e] == l && BlockWanted(ctx, e)) {
        if (ns[e] > 32 || nsep[e] > 16) ctx->level_big[l] = 1;
        if (panel_bytes(e) > kLdsLimit) {
          huge.push_back(e);
          big_ws = std::max(big_ws, (size_t)nsep[e] * nsep[e] + nsep[e] + 1);
          if (ctx->use_ldlt) big_ws = std::max(big_ws, panel_bytes(e) / sizeof(double) + 2);  // the panel image of the LDLT kernel
          continue;
        }
        ctx->level_sn.push_back(e);
        ctx->chol_lds = std::max(ctx->chol_lds, panel_bytes(e));
        // register-shaped LDS image of FactorSupernodeLean: 64 lanes x NSMAX columns
        ctx->chol_lds = std::max(ctx->chol_lds, sizeof(double) * 64 * (size_t)(RegisterShape(ns[e], nsep[e]) >> 8));
      }
    ctx->level_nh[l] = (int)ctx->level_sn.size() - ctx->level_ptr[l];
    // segments: supernodes of a level are independent, so their order inside it is free
    std::stable_sort(ctx->level_sn.begin() + ctx->level_ptr[l], ctx->level_sn.end(),
                     [&](int a, int b) { return seg_key(a) < seg_key(b); });
    for (int e : huge) ctx->level_sn.push_back(e);
    ctx->level_ptr[l + 1] = (int)ctx->level_sn.size();
  }
  // Inside a segment, supernodes that read the solution of the same supernode of the level above
  // sit next to each other (tree_backward_pair hands them to one workgroup); top-down, so that
  // the level above already has its final order.
  {
    std::vector<int> pos_of(K, -1), key(K, 0);
    for (int l = nlev - 2; l >= 0; l--) {
      for (int pos = ctx->level_ptr[l + 1]; pos < ctx->level_ptr[l + 2]; pos++) pos_of[ctx->level_sn[pos]] = pos;
      const auto first = ctx->level_sn.begin() + ctx->level_ptr[l], last = first + ctx->level_nh[l];
      for (auto it = first; it != last; ++it) {
        int best = INT_MAX;
        for (int v : L.separators[*it]) {
          const int p = L.var_to_sn[v];
          if (ctx->t_level[p] == l + 1 && pos_of[p] >= 0) best = std::min(best, pos_of[p]);
        }
        key[*it] = best;
      }
      std::stable_sort(first, last, [&](int a, int b) {
        return std::make_tuple(seg_key(a), key[a]) < std::make_tuple(seg_key(b), key[b]);
      });
    }
  }
  if (big_ws > 0) {
    CXK_DEMAND(ctx->world <= 1, "supernodes beyond LDS are single-GPU for now");
    CXK_TRY(ctx->big_ws.alloc(big_ws));
    // (CXK_NO_BIG_DATAFLOW=1: the host-driven panel loop, for comparison)
    if (!sw.no_big_dataflow) CXK_TRY(ctx->big_flags.alloc(2 * kBigCholMaxBlocks, true));
  }
  CXK_DEMAND(ctx->chol_lds <= kLdsLimit,
             "internal error: a supernode routed to the LDS kernels does not fit LDS");
  CXK_TRY(ctx->d_level_sn.upload(ctx->level_sn));
  CXK_TRY(ctx->d_level_ptr.upload(ctx->level_ptr));
  std::vector<SnRec>& recs = ctx->h_recs;
  recs.assign(ctx->level_sn.size(), SnRec{});
  for (size_t pos = 0; pos < recs.size(); pos++) {
    const int e = ctx->level_sn[pos];
    SnRec& r = recs[pos];
    r.p = e;
    r.ns = ns[e];
    r.nsep = nsep[e];
    r.start = ctx->t_start[e];
    r.tg_beg = u.tg_ptr[e];
    r.tg_end = u.tg_ptr[e + 1];
    r.bs_beg = bo.ptr[e];
    r.bs_end = bo.ptr[e + 1];
    r.diag_off = L.diag_off[e];
    r.offd_off = L.offd_off[e];
    r.upd_off = u.upd_off[e];
    r.updb_off = u.updb_off[e];
    r.ubase = u.ubase[e];
    r.m = u.m[e];
    r.fbase = u.fbase[e];
    r.mf = u.mf[e];
    r.nsep_inline = 0;
    const int cnt = r.bs_end - r.bs_beg;
    if (cnt <= 8 && N < (1 << 26)) {
      r.nsep_inline = cnt;
      for (int q = 0; q < cnt; q++) r.sep[q] = bo.row[r.bs_beg + q] | (bo.c[r.bs_beg + q] << 26);
    }
  }
  CXK_TRY(ctx->p_rec.upload(recs));
  ctx->level_segs.assign(nlev, {});
  ctx->level_lean.assign(nlev, 0);
  for (int l = 0; l < nlev; l++) {
    const int first = ctx->level_ptr[l], last = first + ctx->level_nh[l];
    bool all = ctx->level_nh[l] == ctx->level_ptr[l + 1] - ctx->level_ptr[l] && last > first;
    for (int pos = first; pos < last; pos++) {
      const int e = ctx->level_sn[pos];
      auto& segs = ctx->level_segs[l];
      const int sh = RegisterShape(ns[e], nsep[e]);
      const bool fast = seg_fast(e), inl = seg_inline(e);
      if (segs.empty() || segs.back().shape != sh || segs.back().fast != fast || segs.back().inl != inl) {
        cxk_context::LevelSeg sg;
        sg.begin = pos;
        sg.shape = sh;
        sg.fast = fast;
        sg.inl = inl;
        segs.push_back(sg);
      }
      segs.back().end = pos + 1;
      all = all && sh > 0 && fast && inl;
    }
    ctx->level_lean[l] = all;
    if (sw.debug_levels) {
      fprintf(stderr, "level %d:", l);
      for (auto& sg : ctx->level_segs[l])
        fprintf(stderr, " [%d x <%d,%d>%s%s]", sg.end - sg.begin, sg.shape >> 8, sg.shape & 255, sg.fast ? " fast" : "", sg.inl ? " inline" : "");
      fprintf(stderr, " + %d beyond LDS\n", ctx->level_ptr[l + 1] - ctx->level_ptr[l] - ctx->level_nh[l]);
    }
  }
  return CXK_SUCCESS;
}

// The chain at the top: from the top level down while each level holds ONE lean supernode of at
// most two register shapes, not below floor_level and at most max_len levels.  Returns the lowest
// level of the chain (nlev: none) and its shapes, *sa < *sb when there are two (*sb = 0: one).
int FindChain(const cxk_context* ctx, int floor_level, int max_len, int* sa, int* sb) {
  const int nlev = ctx->nlev;
  int c0 = nlev, a = 0, b = 0;
  while (c0 > floor_level && nlev - c0 < max_len) {
    const int l = c0 - 1;
    if (ctx->level_ptr[l + 1] - ctx->level_ptr[l] != 1 || !ctx->level_lean[l]) break;
    const int sh = ctx->level_segs[l][0].shape;
    if (a == 0 || sh == a) {
      a = sh;
    } else if (b == 0 || sh == b) {
      b = sh;
    } else {
      break;
    }
    c0--;
  }
  if (b != 0 && b < a) std::swap(a, b);
  *sa = a;
  *sb = b;
  return c0;
}

// ---- narrow top of the tree: trailing levels that hold few supernodes are swept by one workgroup
// (levels separated by a workgroup barrier instead of a kernel boundary); never below the cut.
// Then the chain at the top (Cholesky, top swept level by level).
void PlanTopAndChain(cxk_context* ctx, const PlanSwitches& sw) {
  const int nlev = ctx->nlev;
  const bool sharded = ctx->world > 1;
  const int floor_level = sharded ? ctx->cut_level : 0;  // the chain stays inside the replicated top
  int top = nlev;
  while (top > 0 && ctx->level_ptr[top] - ctx->level_ptr[top - 1] <= 8 && !ctx->level_big[top - 1]) top--;
  if (sharded) top = std::max(top, ctx->cut_level);
  if (ctx->use_ldlt) top = nlev;  // LDLT sweeps run level by level, one workgroup per supernode
  // A short top whose levels all have a shape-specialised kernel is swept level by level as
  // well: the lean per-level launches (one memory round trip per step) measured faster than the
  // generic one-workgroup sweep (C4: 24 -> 2 x (6.0 + 3.6) us).  Long narrow tops (chains) keep
  // the one-workgroup sweep: there a kernel boundary per step would dominate.
  if (!ctx->no_lean && !sw.keep_top && top < nlev && nlev - top <= kSplitTopLevels) {
    bool all = true;
    for (int l = top; l < nlev; l++) all = all && ctx->level_lean[l];
    if (all) top = nlev;
  }
  // A narrow top that is a pure chain -- one lean supernode per level, at most two shapes -- goes to
  // the chain kernel whatever its length (one launch of one wavefront, records prefetched, no
  // workgroup barriers): BASELINE config 3 as the reference arranges it is 5000 such levels.
  if (!ctx->use_ldlt && !ctx->no_lean && !sw.no_chain && !sw.keep_top && top < nlev) {
    int sa, sb;
    const int c0 = FindChain(ctx, floor_level, INT_MAX, &sa, &sb);
    if (c0 <= top && nlev - c0 >= 2 && ChainPairCompiled(sa, sb)) top = nlev;
  }
  ctx->top_level = top;
  ctx->chain_level = nlev;
  Verdict v;
  v.check(!ctx->use_ldlt && !ctx->no_lean && !sw.no_chain, "LDLT, generic kernels or CXK_NO_CHAIN");
  v.check(top == nlev, "the narrow top is swept by one workgroup");
  if (v.ok) {
    int sa, sb;
    const int c0 = FindChain(ctx, floor_level, kChainMaxLevels, &sa, &sb);
    v.check(nlev - c0 >= 2, "fewer than two levels of one lean supernode at the top");
    v.check(ChainPairCompiled(sa, sb), "no instance for the pair of shapes");
    if (v.ok) {
      ctx->chain_level = c0;
      ctx->chain_a = sa;
      ctx->chain_b = sb == 0 ? sa : sb;
    }
  }
  if (!v.ok) v.refuse(sw, "chain");
}

// ---- pairs of downward levels, from the leaves up: both one lean segment, every lower supernode
// reads at most one supernode of the upper level, and those that read the same one are consecutive
int PlanBackPairs(cxk_context* ctx, const PlanSwitches& sw) {
  const Layout& L = ctx->lay;
  const int nlev = ctx->nlev;
  ctx->back_pairs.clear();
  ctx->back_pairs.resize(nlev);
  if (ctx->use_ldlt || ctx->no_lean || ctx->top_level != nlev || sw.no_back_pairs) return CXK_SUCCESS;
  const int up_end = ctx->chain_level < nlev ? ctx->chain_level : nlev;
  auto plain = [&](int l) {
    return ctx->level_lean[l] && !ctx->level_big[l] && ctx->level_segs[l].size() == 1 &&
           ctx->level_nh[l] == ctx->level_ptr[l + 1] - ctx->level_ptr[l];
  };
  std::vector<int> pos_of(ctx->md.K, -1);
  for (int l = 0; l + 1 < up_end;) {
    bool ok = plain(l) && plain(l + 1);
    std::vector<BackPairEntry> tab;
    if (ok) {
      for (int pos = ctx->level_ptr[l + 1]; pos < ctx->level_ptr[l + 2]; pos++) pos_of[ctx->level_sn[pos]] = pos;
      std::vector<int> dep(ctx->level_ptr[l + 1] - ctx->level_ptr[l], -1);
      for (int pos = ctx->level_ptr[l]; pos < ctx->level_ptr[l + 1] && ok; pos++) {
        int d = -1;
        for (int v : L.separators[ctx->level_sn[pos]]) {
          const int p = L.var_to_sn[v];
          if (ctx->t_level[p] != l + 1) continue;
          if (pos_of[p] < 0 || (d >= 0 && d != pos_of[p])) ok = false;
          d = pos_of[p];
        }
        dep[pos - ctx->level_ptr[l]] = d;
      }
      // runs of equal dependence; a parent's children must form ONE run
      std::vector<char> seen(ctx->level_ptr[l + 2] - ctx->level_ptr[l + 1], 0);
      for (int i = 0; i < (int)dep.size() && ok;) {
        int j = i;
        while (j < (int)dep.size() && dep[j] == dep[i]) j++;
        if (dep[i] >= 0) {
          char& sn = seen[dep[i] - ctx->level_ptr[l + 1]];
          if (sn) ok = false;
          sn = 1;
          tab.push_back(BackPairEntry{dep[i], ctx->level_ptr[l] + i, j - i, 0});
        } else {
          for (int q = i; q < j; q += 8) tab.push_back(BackPairEntry{-1, ctx->level_ptr[l] + q, std::min(8, j - q), 0});
        }
        i = j;
      }
      // a supernode of the upper level nobody below reads (cannot happen by the definition of a
      // level; kept for safety): solved by a workgroup without children
      for (size_t q = 0; q < seen.size() && ok; q++)
        if (!seen[q]) tab.push_back(BackPairEntry{ctx->level_ptr[l + 1] + (int)q, ctx->level_ptr[l], 0, 0});
    }
    if (ok) {
      auto bp = std::make_unique<cxk_context::BackPair>();
      bp->nwg = (int)tab.size();
      bp->shape_p = ctx->level_segs[l + 1][0].shape;
      bp->shape_c = ctx->level_segs[l][0].shape;
      CXK_TRY(bp->tab.upload(tab));
      if (sw.debug_levels) fprintf(stderr, "backward pair: levels %d + %d in %d workgroups\n", l + 1, l, bp->nwg);
      ctx->back_pairs[l + 1] = std::move(bp);
      l += 2;
    } else {
      l += 1;
    }
  }
  return CXK_SUCCESS;
}

// ---- solve-only sweeps: does every forward launch run a lean kernel (then the right-hand side is
// formed inside them, RhsIn)?  Levels below the chain must be all-lean single launches, the
// rest must be the chain (no one-workgroup top, no supernode beyond LDS).
void PlanLeanSolve(cxk_context* ctx) {
  const int nlev = ctx->nlev;
  bool all = ctx->world <= 1 && !ctx->use_ldlt && !ctx->no_lean && ctx->top_level == nlev;
  const int up_end = ctx->chain_level < nlev ? ctx->chain_level : nlev;
  for (int l = 0; l < up_end && all; l++) {
    all = ctx->level_lean[l] && !ctx->level_big[l] &&
          ctx->level_nh[l] == ctx->level_ptr[l + 1] - ctx->level_ptr[l] && ctx->level_segs[l].size() <= 2;
  }
  ctx->forward_all_lean = all && nlev >= 1;
}

// ---- assembly folded into the first factor level.  Taken when level 0 is ONE segment of a
// register shape with dense pulls, launched on its own (not part of a chain / dense top), and
// every supernode in it is a leaf whose panel entries and right-hand-side rows have exactly one
// source each, all in the Schur block of its own constraint, at positions pos[row] -- the
// leaves of a clique tree.  Those supernodes then read G(max(pos_r, pos_c), min(..)) themselves
// and the gather lists shrink to what the levels above need.
int PlanFusedAssembly(cxk_context* ctx, const PlanSwitches& sw, const AsmGather& ag, const ResidGather& rg,
                      const UpdateSlots& u) {
  const MatrixData& md = ctx->md;
  const Layout& L = ctx->lay;
  const int N = md.N, nlev = ctx->nlev;
  ctx->fused_asm = false;
  Verdict v;
  v.check((ctx->world <= 1 || ctx->cut_level >= 1) && !ctx->use_ldlt && !ctx->no_lean && !sw.no_fused_asm,
          "sharded without subtrees, LDLT, generic kernels or CXK_NO_FUSED_ASM");
  v.check(!HasFactoredLmi(ctx), "an LMI given by factors");
  v.check(nlev >= 2 && (ctx->level_segs[0].size() == 1 || ctx->level_segs[0].size() == 2) && ctx->level_lean[0] &&
              ctx->top_level >= 1 && ctx->chain_level >= 1 && ctx->level_segs[0][0].shape != 0 && 4 * ctx->chol_lds <= kLdsLimit,
          "level 0 is not a lean launch of its own");
  if (!v.ok) return v.refuse(sw, "fused assembly");
  const int first = ctx->level_ptr[0], cnt0 = ctx->level_nh[0];
  std::vector<AsmRec> arecs(cnt0);
  std::vector<char> slab_own(ag.rec.size(), 0), var_own(N, 0);
  bool ok = cnt0 > 0 && cnt0 == ctx->level_ptr[1] - first;
  for (int q = 0; q < cnt0 && ok; q++) {
    const int e = ctx->level_sn[first + q];
    const int i = md.clique_order[e];
    const int m = ctx->cons[i].m;
    const IntList& r = md.supernodes_pos[e];
    const IntList& sp = md.separators_pos[e];
    const int nse = (int)r.size(), nsp = (int)sp.size();
    ok = nse == ctx->t_ns[e] && nsp == ctx->t_nsep[e] && nse + nsp <= 72 && m <= 255 && ctx->owned[i] &&
         u.tg_ptr[e + 1] == u.tg_ptr[e] && u.mf[e] == 0;
    AsmRec& ar = arecs[q];
    memset(&ar, 0, sizeof(ar));
    ar.g_off = ctx->g_off[i];
    ar.r_off = ctx->r_off[i];
    ar.m = m;
    for (int a = 0; a < nse && ok; a++) {
      ok = r[a] >= 0 && r[a] < m;
      ar.pos[a] = (unsigned char)r[a];
    }
    for (int a = 0; a < nsp && ok; a++) {
      ok = sp[a] >= 0 && sp[a] < m;
      ar.pos[nse + a] = (unsigned char)sp[a];
    }
    auto single = [&](int64_t off, int pa, int pb) {  // the slab entry has the one source G(pa, pb)
      const int t = ag.entry_of[off];
      if (t < 0) return false;
      const GatherRec& g = ag.rec[t];
      const int hi = std::max(pa, pb), lo = std::min(pa, pb);
      if (g.extra != 0 || g.first != ar.g_off + hi + (int64_t)lo * m) return false;
      slab_own[t] = 1;
      return true;
    };
    for (int j = 0; j < nse && ok; j++)
      for (int i2 = j; i2 < nse && ok; i2++) ok = single(L.diag_off[e] + (int64_t)j * nse + i2, r[i2], r[j]);
    for (int j = 0; j < nsp && ok; j++)
      for (int i2 = 0; i2 < nse && ok; i2++) ok = single(L.offd_off[e] + (int64_t)j * nse + i2, r[i2], sp[j]);
    for (int a = 0; a < nse && ok; a++) {
      const int pvar = ctx->t_start[e] + a;
      ok = rg.per[pvar].size() == 1 && rg.per[pvar][0] == ar.r_off + r[a];
      var_own[pvar] = 1;
    }
  }
  v.check(ok, "a level-0 supernode that is not a leaf with single sources in its own constraint's block");
  if (!v.ok) return v.refuse(sw, "fused assembly");
  std::vector<GatherRec> g2;
  for (size_t t = 0; t < ag.rec.size(); t++)
    if (!slab_own[t]) g2.push_back(ag.rec[t]);
  std::vector<ResidRec> r2;
  std::vector<int> v2;
  for (int pvar = 0; pvar < N; pvar++)
    if (!var_own[pvar]) {
      r2.push_back(rg.rec[pvar]);
      v2.push_back(pvar);
    }
  ctx->as_T2 = (int64_t)g2.size();
  ctx->rs_N2 = (int)v2.size();
  if (g2.empty()) g2.push_back(GatherRec{0, -1, 0, 0});
  if (v2.empty()) {
    r2.push_back(ResidRec{-1, 0, 0});
    v2.push_back(0);
  }
  CXK_TRY(ctx->asm_rec.upload(arecs));
  CXK_TRY(ctx->as_rec2.upload(g2));
  CXK_TRY(ctx->rs_rec2.upload(r2));
  CXK_TRY(ctx->rs_var2.upload(v2));
  ctx->fused_asm = true;
  return CXK_SUCCESS;
}

// ---- the whole tree in one launch (tree_fused.hip).  Taken when every supernode has a register
// kernel (at most two shapes) with dense pulls and an inline separator list, sits alone in its
// constraint's Schur block at non-negative positions (no fill-in rows), its entries take their
// first source from that block, the lists of further sources fit the dense slots, and the grid
// is resident at once (the way back down waits for HIGHER positions).

// The tables of the whole-tree launch (tree_fused.h): kFusedRecWords words per position, the
// entries / variables with further sources, and where each supernode publishes
struct FusedTables {
  std::vector<int> recs, xreg, pub;
  std::vector<unsigned> img;  // load images, img_stride dwords per position (0: the launch has none)
  int img_stride = 0;
  std::vector<long long> xsrc, rsrc;
};

// The frames of RegisterShape are padded for most trees (config 4: 15 + 5 in <16, 8>, its root's 20 columns in
// <24, 0>), and every padding column is a multiply-add per pivot, every padding pivot a step of the root's back
// substitution.  Per frame of the pair: the tightest compiled frame (kFusedFrames) that holds every supernode the
// launch sends there -- <NA, SA> takes what fits it, <NB, SB> the rest -- with the same rows per lane (the same NSMAX
// wherever a supernode has separator rows: the image locations tg_reg / xreg count from it).  The pair is taken
// only when an instance exists for it; padding contributes exact zeros and unit pivots, so the results are the
// same bits in either pair (CXK_FUSED_PADDED_FRAMES=1 keeps the padded one).
void TightFrames(const cxk_context* ctx, int* sa, int* sb) {
  const int pa = *sa, pb = *sb;
  int mn[2] = {0, 0}, ms[2] = {0, 0};
  for (int e : ctx->level_sn) {
    const int n = ctx->t_ns[e], s = ctx->t_nsep[e];
    const int g = (pa == pb || (n <= (pa >> 8) && s <= (pa & 255))) ? 0 : 1;
    mn[g] = std::max(mn[g], n);
    ms[g] = std::max(ms[g], s);
  }
  int tight[2] = {pa, pb};
  for (int g = 0; g < 2; g++) {
    const int padded = g == 0 ? pa : pb;
    for (int f : kFusedFrames)
      if (mn[g] <= (f >> 8) && ms[g] <= (f & 255) && (f >> 8) <= (padded >> 8) && (f & 255) <= (padded & 255) &&
          (ms[g] == 0 || (f >> 8) == (padded >> 8))) {
        tight[g] = f;
        break;
      }
  }
  if (pa == pb) tight[1] = tight[0];
  // (a supernode of the second frame must not fit the first: it did not fit the padded one, which holds the tight one)
  if (tight[0] <= tight[1] && FusedTreeCompiled(tight[0], tight[1])) {
    *sa = tight[0];
    *sb = tight[1];
  }
}

// The pair of register shapes the launch runs on (*sa <= *sb); returns whether the program is ONE
// dense supernode of 33 .. 64 columns (BASELINE config 2: 50): the wide instances of the same
// launch (tree_fused.hip, ElimWide)
bool FusedTreeShapes(const cxk_context* ctx, const PlanSwitches& sw, const UpdateSlots& u, Verdict& v, int* sa, int* sb) {
  const int nlev = ctx->nlev;
  const std::vector<int>& ns = ctx->t_ns;
  const int cnt_all = (int)ctx->level_sn.size();
  const bool wide_single = v.ok && ctx->world <= 1 && cnt_all == 1 && ctx->md.K >= 1 && ns[ctx->level_sn[0]] > 32 &&
                           ns[ctx->level_sn[0]] <= 64 && ctx->t_nsep[ctx->level_sn[0]] == 0 && !sw.no_fused_wide;
  if (wide_single) {
    *sa = *sb = ((ns[ctx->level_sn[0]] + 7) / 8 * 8) << 8;
    return true;
  }
  // at most two register shapes; a shape without separator columns <N, 0> runs on <N, S> where
  // the tree has one (same rows per lane: the pull locations tg_reg are the same)
  std::vector<int> shapes;
  for (int l = 0; l < nlev && v.ok; l++) {
    if (ctx->level_ptr[l + 1] == ctx->level_ptr[l]) continue;  // (a level this rank has no supernode on)
    v.ok = !ctx->level_big[l] && ctx->level_nh[l] == ctx->level_ptr[l + 1] - ctx->level_ptr[l];
    // (the whole-tree kernels take pull lists of any length up to kFusedMaxSlots, kFastSlots at a
    // time: a level needs a register shape and inline separator lists, not the level kernels' "fast")
    for (auto& sg : ctx->level_segs[l]) {
      v.ok = v.ok && sg.shape != 0 && sg.inl;
      if (std::find(shapes.begin(), shapes.end(), sg.shape) == shapes.end()) shapes.push_back(sg.shape);
    }
    for (int pos = ctx->level_ptr[l]; pos < ctx->level_ptr[l + 1] && v.ok; pos++) {
      const int e = ctx->level_sn[pos];
      v.ok = u.tg_ptr[e + 1] - u.tg_ptr[e] <= kFastTargets && u.m[e] <= kFusedMaxSlots && u.mf[e] <= kFusedMaxSlots;
    }
  }
  for (size_t i = 0; i < shapes.size(); i++)
    if ((shapes[i] & 255) == 0)
      for (size_t j = 0; j < shapes.size(); j++)
        if (j != i && shapes[i] >= 0 && (shapes[j] >> 8) == (shapes[i] >> 8) && (shapes[j] & 255) > 0) {
          shapes[i] = -1;
          break;
        }
  shapes.erase(std::remove(shapes.begin(), shapes.end(), -1), shapes.end());
  std::sort(shapes.begin(), shapes.end());
  v.note("a level without a register shape, inline separator lists or within the slot limits");
  v.check(!shapes.empty() && shapes.size() <= 2, "more than two register shapes");
  if (v.ok) {
    *sa = shapes[0];
    *sb = shapes.back();
    if (!sw.fused_padded_frames && ctx->world <= 1) TightFrames(ctx, sa, sb);  // (sharded contexts keep the padded pair)
  }
  return false;
}

// The record of every position: the level record (SnRec) in words 0 .., then below the cut the
// supernode's own block (AsmRec) and its entries / variables with further sources, above it
// (the replicated top of a sharded context) where its panel sits in the exchange buffer
void FusedTreeRecords(const cxk_context* ctx, const AsmGather& ag, const ResidGather& rg, const ExchangeLayout& x,
                      int cnt_up, int wide_shape, Verdict& v, FusedTables* ft) {
  const MatrixData& md = ctx->md;
  const Layout& L = ctx->lay;
  const std::vector<int>& ns = ctx->t_ns;
  const std::vector<int>& start = ctx->t_start;
  const int cnt_all = (int)ctx->level_sn.size();
  std::vector<int>& recs = ft->recs;
  recs.assign((size_t)cnt_all * kFusedRecWords, 0);
  for (int pos = 0; pos < cnt_all && v.ok; pos++) {
    const int e = ctx->level_sn[pos];
    const int i = md.clique_order[e];
    const int m = ctx->cons[i].m;
    const IntList& r = md.supernodes_pos[e];
    const IntList& sp = md.separators_pos[e];
    const int nse = (int)r.size(), nsp = (int)sp.size();
    const int nsm = wide_shape ? wide_shape >> 8 : RegisterShape(ns[e], ctx->t_nsep[e]) >> 8;
    int* w = recs.data() + (size_t)pos * kFusedRecWords;
    if (pos >= cnt_up) {
      // the replicated top of a sharded context: the panel comes from the exchange buffer
      if (!v.check(ctx->sn_top[e] && nsm > 0 && x.xs_base[e] >= 0 && ctx->n_xs < (int64_t)INT32_MAX,
                   "a top supernode without a register kernel"))
        break;
      memcpy(w, &ctx->h_recs[pos], sizeof(SnRec));
      w[32] = (int)(x.xs_base[e] & 0xffffffffll);
      w[33] = (int)(x.xs_base[e] >> 32);
      w[34] = x.xv_base[e];
      w[63] = ctx->t_level[e];
      continue;
    }
    if (!v.check(nse == ns[e] && nsp == ctx->t_nsep[e] && nse + nsp <= 72 && m <= 254 && ctx->owned[i] && nsm > 0,
                 "a supernode that is not its constraint's own block"))
      break;
    memcpy(w, &ctx->h_recs[pos], sizeof(SnRec));
    AsmRec ar;
    memset(&ar, 0, sizeof(ar));
    ar.g_off = ctx->g_off[i];
    ar.r_off = ctx->r_off[i];
    ar.m = m;
    for (int a = 0; a < nse && v.ok; a++) {
      v.ok = r[a] >= 0 && r[a] < m;
      ar.pos[a] = (unsigned char)r[a];
    }
    v.note("a fill-in variable among the supernode's own (position -1)");
    // separator rows the constraint does not contain (structural fill: the deferred variables of a
    // segmented chain): position 255, entries that start as zeros (AsmRec::pad_ flags the record)
    for (int a = 0; a < nsp && v.ok; a++) {
      v.ok = sp[a] < m;
      ar.pos[nse + a] = sp[a] < 0 ? (unsigned char)255 : (unsigned char)sp[a];
      if (sp[a] < 0) ar.pad_ = 1;
    }
    if (!v.ok) break;
    memcpy(w + 32, &ar, sizeof(AsmRec));
    // entries with further sources, in the order of the panel (columns of the diagonal block, then
    // the off block): (image location, sources)
    std::vector<std::pair<int, std::vector<int64_t>>> extra;
    auto visit = [&](int64_t off, int pa, int pb, int reg) {
      const int t = ag.entry_of[off];
      if (t < 0) return false;
      const GatherRec& g = ag.rec[t];
      const int hi = std::max(pa, pb), lo = std::min(pa, pb);
      if (pa < 0 || pb < 0) {  // a fill-in row: no source in the own block
        if (g.first >= 0) return false;
      } else if (g.first != ar.g_off + hi + (int64_t)lo * m) {
        return false;
      }
      if (g.extra > 0) {
        extra.emplace_back(reg, std::vector<int64_t>(ag.src.begin() + g.beg, ag.src.begin() + g.beg + g.extra));
      }
      return true;
    };
    for (int j = 0; j < nse && v.ok; j++)
      for (int i2 = j; i2 < nse && v.ok; i2++) v.ok = visit(L.diag_off[e] + (int64_t)j * nse + i2, r[i2], r[j], 64 * j + i2);
    for (int j = 0; j < nsp && v.ok; j++)
      for (int i2 = 0; i2 < nse && v.ok; i2++) v.ok = visit(L.offd_off[e] + (int64_t)j * nse + i2, r[i2], sp[j], 64 * i2 + nsm + j);
    v.note("an entry whose first source is not the own block");
    size_t mx = 0;
    for (auto& xe : extra) mx = std::max(mx, xe.second.size());
    v.check(extra.size() <= (size_t)kFusedExtraTargets && mx <= (size_t)kFusedExtraMax,
            "too many entries with further sources / too many sources");
    // variables that several constraints share: all their sources, in the gather's order
    size_t mr = 0;
    for (int a = 0; a < nse && v.ok; a++) {
      const auto& lst = rg.per[start[e] + a];
      if (lst.size() == 1)
        v.ok = lst[0] == ar.r_off + r[a];
      else
        v.ok = !lst.empty() && std::find(lst.begin(), lst.end(), ar.r_off + r[a]) != lst.end();
      if (lst.size() > 1) mr = std::max(mr, lst.size());
    }
    v.note("a variable whose sources do not include the own constraint");
    v.check(mr <= (size_t)kFusedExtraMax, "a variable shared by more than 64 constraints");
    if (!v.ok) break;
    const int64_t xbase = (int64_t)ft->xsrc.size();
    w[56] = (int)ft->xreg.size();
    w[57] = (int)extra.size();
    w[58] = (int)mx;
    w[59] = (int)ft->rsrc.size();
    w[60] = (int)mr;
    w[61] = (int)(xbase & 0xffffffffll);
    w[62] = (int)(xbase >> 32);
    w[63] = ctx->t_level[e];
    for (auto& xe : extra) {
      ft->xreg.push_back(xe.first);
      for (size_t q2 = 0; q2 < mx; q2++) ft->xsrc.push_back(q2 < xe.second.size() ? (long long)xe.second[q2] : -1ll);
    }
    if (mr > 0)
      for (int a = 0; a < nse; a++) {
        const auto& lst = rg.per[start[e] + a];
        for (size_t q2 = 0; q2 < mr; q2++) ft->rsrc.push_back(lst.size() > 1 && q2 < lst.size() ? (long long)lst[q2] : -1ll);
      }
    v.ok = ft->rsrc.size() < (size_t)INT32_MAX && ft->xreg.size() < (size_t)INT32_MAX;
  }
}

// A supernode's published values go to the supernodes that own its separator variables: all of
// them must sit at higher positions (waits go to lower positions on the way up).  Forward values
// are numbered behind the n_upd Schur-value slots.
void FusedTreePublished(const cxk_context* ctx, const UpdateSlots& u, const std::vector<int>& pos_of, size_t n_upd,
                        size_t n_updb, Verdict& v, FusedTables* ft) {
  const Layout& L = ctx->lay;
  const int cnt_all = (int)ctx->level_sn.size();
  for (int pos = 0; pos < cnt_all && v.ok; pos++) {
    const int e = ctx->level_sn[pos];
    for (int x : L.separators[e]) v.check(pos_of[L.var_to_sn[x]] > pos, "a consumer at a lower position");
  }
  v.ok = v.ok && n_upd + n_updb + 8 < (size_t)INT32_MAX;
  for (int pos = 0; pos < cnt_all && v.ok; pos++) {
    const int e = ctx->level_sn[pos];
    const int nsep = ctx->t_nsep[e];
    int* w = ft->recs.data() + (size_t)pos * kFusedRecWords;
    w[21] = w[22] = 0;
    w[23] = (int)ft->pub.size();
    for (int64_t t = 0; t < (int64_t)nsep * (nsep + 1) / 2; t++) ft->pub.push_back(u.pub_dst[(size_t)(u.upd_off[e] + t)]);
    for (int c = 0; c < nsep; c++) ft->pub.push_back((int)n_upd + u.pubb_dst[(size_t)(u.updb_off[e] + c)]);
  }
}

// The load image of every position below the cut (tree_fused.h, FusedImgLayout): what FusedSupernode's load phase
// would derive from the record -- where each lane finds each entry of its panel, which entries do not exist, where
// its row of the right-hand side and of the factor sits, where the published values go and where they are picked up
// behind the elimination -- is structure, fixed with the plans.  Entries that do not exist point at the +0.0 behind
// the last block of G, a padding pivot's diagonal at the 1.0 behind that (AllocateSystemBuffers leaves room, the
// caller writes the two words).  Offsets are 32-bit: a context whose G, AWc or hand-off slots lie beyond that keeps
// the level kernels.
void FusedTreeLoadImages(const cxk_context* ctx, int sa, int sb, int cnt_up, size_t n_upd, size_t n_updb, Verdict& v,
                         FusedTables* ft) {
  const int na = sa >> 8, ssa = sa & 255, nb = sb >> 8, ssb = sb & 255;
  if (na > 32 || nb > 32) return;  // (the wide frames keep the computed load phase)
  const FusedImgLayout ly = FusedImgLayoutOf(na, ssa, nb, ssb);
  const int K = (int)ctx->cons.size();
  const int64_t g_end = ctx->g_off[K - 1] + (int64_t)ctx->cons[K - 1].m * ctx->cons[K - 1].m;
  const int64_t go = (int64_t)ctx->G.n - 2;  // the two constants
  const int64_t ro = ctx->r_off[K - 1] + ctx->cons[K - 1].m;
  if (!v.check(go >= g_end && 8 * (go + 2) <= (int64_t)UINT32_MAX && ro < (int64_t)INT32_MAX &&
                   ctx->md.N < INT32_MAX - 64 && n_upd + 3 * n_updb + 8 < (size_t)INT32_MAX,
               "offsets beyond the 32 bits of the load image"))
    return;
  const unsigned zero_at = (unsigned)(8 * go), one_at = (unsigned)(8 * (go + 1));
  const int cnt_all = (int)ctx->level_sn.size();
  ft->img_stride = ly.stride;
  ft->img.assign((size_t)cnt_all * ly.stride, 0u);
  for (int pos = 0; pos < cnt_up && v.ok; pos++) {
    const int* w = ft->recs.data() + (size_t)pos * kFusedRecWords;
    unsigned* im = ft->img.data() + (size_t)pos * ly.stride;
    SnRec sr;
    AsmRec ar;
    memcpy(&sr, w, sizeof(SnRec));
    memcpy(&ar, w + 32, sizeof(AsmRec));
    const int ns = sr.ns, s = sr.nsep;
    const bool in_a = sa == sb || (ns <= na && s <= ssa);  // (FitsFrame, tree_fused.hip)
    const int nsm = in_a ? na : nb, smx = in_a ? ssa : ssb;
    if (!v.check(ns >= 1 && ns <= nsm && s <= smx && ns <= 0xffff, "a supernode beyond its frame")) break;
    const unsigned rel = (unsigned)(sr.offd_off - sr.diag_off);
    auto entry = [&](int pa, int pb) {
      const int hi = std::max(pa, pb), lo = std::min(pa, pb);
      return (unsigned)(8 * (ar.g_off + hi + (int64_t)lo * ar.m));
    };
    for (int row = 0; row < ly.rows; row++) {
      unsigned* o = im + (size_t)row * ly.nc;
      unsigned* l = im + ly.l_at + 4 * row;
      for (int j = 0; j < ly.nc; j++) o[j] = zero_at;
      l[0] = (unsigned)(ar.r_off + ar.pos[0]);
      l[1] = (unsigned)sr.start;
      l[2] = 0u;
      l[3] = 1u;  // st = 1, lim = 0
      const int c = row - nsm;
      if (row < ns) {
        for (int j = 0; j <= row; j++) o[j] = entry(ar.pos[row], ar.pos[j]);
        l[0] = (unsigned)(ar.r_off + ar.pos[row]);
        l[1] = (unsigned)(sr.start + row);
        l[2] = (unsigned)row;
        l[3] = (unsigned)ns | (unsigned)(row + 1) << 16;
      } else if (c >= 0 && c < s) {
        if (ar.pos[ns + c] != 255)  // (255: structural fill, the row starts as zeros)
          for (int j = 0; j < ns; j++) o[j] = entry(ar.pos[ns + c], ar.pos[j]);
        l[2] = rel + (unsigned)(c * ns);
        l[3] = 1u | (unsigned)ns << 16;
      } else if (row < nsm) {
        o[row] = one_at;  // a padding pivot
      }
    }
    // published values, numbered as for three right-hand sides
    const int npairs = s * (s + 1) / 2, nv3 = npairs + 3 * s;
    const int rl = FusedRhsLane(nsm, smx);
    if (!v.check(nv3 <= ly.ul, "more published values than the load image holds")) break;
    for (int t = 0; t < nv3; t++) {
      const int tq = t >= npairs + s ? (t - npairs) / s : 0;
      const int tk = t - tq * s;  // the value of right-hand side 0 it sits behind
      int k = 0, rem = t < npairs ? t : 0;
      while (k < s && rem >= s - k) {
        rem -= s - k;
        k++;
      }
      const int kk = t < npairs ? k : tk - npairs, cc = t < npairs ? k + rem : smx + tq;
      const unsigned as_col = (unsigned)(nsm + kk) | (unsigned)cc << 8;
      const unsigned as_row = (rl >= 0 && t >= npairs) ? ((unsigned)(rl + tq) | (unsigned)kk << 8) : as_col;
      im[ly.u_at + 2 * t] = (unsigned)(ft->pub[(size_t)w[23] + tk] + tq * (int)n_updb);
      im[ly.u_at + 2 * t + 1] = as_row | as_col << 16 | (tq > 0 ? 1u << 31 : 0u);
    }
  }
}

// Which workgroup takes which supernode.  Every wavefront of the launch is resident (no order is needed
// for progress) and the dispatcher deals workgroups round-robin over the 8 XCDs (workgroup b on XCD
// b mod 8: tools/xcc_placement_bench.hip -- a speed assumption only).  A hand-off between wavefronts of
// one XCD is 0.1 - 0.3 us shorter than one across the fabric (MI355X_MICROARCH.md, handoff-1to1), and
// the launch is nine hand-offs deep: the supernodes are dealt in depth-first order of the tree, an
// eighth of them per XCD, so that a supernode mostly sits with its children; within an XCD the level
// order stays (leaves first: they have the most to load).  (Within a level, the supernodes with the longest
// chain of ancestors first -- C4: the 415 leaves at depth four -- measured nothing: DESIGN 4.3.1.)
void DealOverXcds(const cxk_context* ctx, const std::vector<int>& pos_of, FusedTables* ft) {
  std::vector<int>* recs = &ft->recs;
  const Layout& L = ctx->lay;
  const int cnt_all = (int)ctx->level_sn.size();
  std::vector<std::vector<int>> kids(cnt_all);
  std::vector<int> roots;
  for (int pos = 0; pos < cnt_all; pos++) {
    int par = INT32_MAX;
    for (int v : L.separators[ctx->level_sn[pos]]) par = std::min(par, pos_of[L.var_to_sn[v]]);
    if (par == INT32_MAX)
      roots.push_back(pos);
    else
      kids[par].push_back(pos);
  }
  std::vector<int> dfs, stack(roots.rbegin(), roots.rend());
  dfs.reserve(cnt_all);
  while (!stack.empty()) {
    const int u = stack.back();
    stack.pop_back();
    dfs.push_back(u);
    for (auto it = kids[u].rbegin(); it != kids[u].rend(); ++it) stack.push_back(*it);
  }
  if ((int)dfs.size() != cnt_all) return;
  std::vector<int> perm(cnt_all, -1);  // workgroup -> position in level order
  size_t at = 0;
  for (int x = 0; x < 8; x++) {
    const int n = (cnt_all - x + 7) / 8;  // workgroups x, x + 8, ... below cnt_all
    std::vector<int> mine(dfs.begin() + at, dfs.begin() + at + n);
    at += n;
    std::sort(mine.begin(), mine.end());
    for (int i = 0; i < n; i++) perm[8 * i + x] = mine[i];
  }
  std::vector<int> dealt(recs->size());
  for (int b = 0; b < cnt_all; b++)
    memcpy(dealt.data() + (size_t)b * kFusedRecWords, recs->data() + (size_t)perm[b] * kFusedRecWords, sizeof(int) * kFusedRecWords);
  recs->swap(dealt);
  // (a workgroup's load image sits at its index, like its record)
  if (ft->img_stride > 0) {
    std::vector<unsigned> img(ft->img.size());
    for (int b = 0; b < cnt_all; b++)
      memcpy(img.data() + (size_t)b * ft->img_stride, ft->img.data() + (size_t)perm[b] * ft->img_stride, sizeof(unsigned) * ft->img_stride);
    ft->img.swap(img);
  }
}

int PlanFusedTree(cxk_context* ctx, const PlanSwitches& sw, const AsmGather& ag, const ResidGather& rg,
                  const UpdateSlots& u, const ExchangeLayout& x) {
  const int N = ctx->md.N, nlev = ctx->nlev;
  const bool sharded = ctx->world > 1;
  ctx->fused_tree = false;
  ctx->fused_sweep = false;
  ctx->fused_shard = false;
  Verdict v;
  // (sharded contexts: the own subtrees up to the cut and, behind the exchange, the replicated top and
  // the way back down -- two launches, tree_fused.h; CXK_NO_FUSED_SHARD=1 keeps the level kernels there)
  v.check((!sharded || (!sw.no_fused_shard && ctx->cut_level >= 1 && ctx->cut_level < nlev)) && !ctx->use_ldlt &&
              !ctx->no_lean && !sw.no_fused_tree && nlev >= 1 && N < (1 << 26),
          "LDLT, generic kernels, CXK_NO_FUSED_TREE / CXK_NO_FUSED_SHARD or no subtrees below the cut");
  v.check(!HasFactoredLmi(ctx), "an LMI given by factors");
  if (!v.ok) return v.refuse(sw, "whole-tree launch");
  const int cnt_all = (int)ctx->level_sn.size();
  const int cnt_up = sharded ? ctx->level_ptr[ctx->cut_level] : cnt_all;  // positions below the cut
  v.check(cnt_all > 0 && cnt_all == ctx->level_ptr[nlev], "a supernode without columns / beyond LDS");
  int sa = 0, sb = 0;
  const bool wide_single = FusedTreeShapes(ctx, sw, u, v, &sa, &sb);
  // (a tree that is one long chain keeps the chain kernel: one wavefront, no hand-offs)
  v.check(nlev <= 64 || cnt_all >= 4 * nlev, "a long chain");
  v.check(FusedTreeCompiled(sa, sb), "no instance for the pair of shapes");
  FusedTables ft;
  FusedTreeRecords(ctx, ag, rg, x, cnt_up, wide_single ? sa : 0, v, &ft);
  const size_t us = (size_t)u.slots + 1 + kPullPad, ubs = (size_t)u.slotsb + 2 + kPullPad;
  std::vector<int> pos_of(ctx->md.K, -1);  // supernode -> position in level order
  for (int pos = 0; pos < cnt_all; pos++) pos_of[ctx->level_sn[pos]] = pos;
  if (v.ok) FusedTreePublished(ctx, u, pos_of, us, ubs, v, &ft);
  if (v.ok) FusedTreeLoadImages(ctx, sa, sb, cnt_up, us, ubs, v, &ft);
  bool split = false;
  if (v.ok) {
    // residency: every workgroup (one wavefront each, one more for the scalars) at once, with a
    // CU's worth of margin per slot count the occupancy query may overstate; a larger tree takes
    // the way up and the way down as two launches (tree_fused.h, FusedTreeMode)
    const int occ = FusedTreeOccupancy(sa, sb, sharded);
    v.check(occ >= 2, "occupancy query failed");
    split = (int64_t)cnt_all + 1 > (int64_t)(occ - 1) * ctx->cus || sw.fused_split;
    if (sharded) {
      // only the top has to be resident at once (tree_fused.h, kFusedShardTop)
      v.check((int64_t)(cnt_all - cnt_up) + 1 <= (int64_t)(occ - 1) * ctx->cus,
              "the replicated top exceeds the resident wavefronts");
      split = false;
    }
  }
  if (v.ok && sharded) {
    // pack tables: per exchange entry / top variable the record of its own-rank sources
    std::vector<GatherRec> xg(x.xs.size() + 1, GatherRec{0, -1, 0, 0});
    for (size_t t = 0; t < x.xs.size() && v.ok; t++) {
      const int et = ag.entry_of[x.xs[t]];
      v.ok = et >= 0;
      if (v.ok) xg[t] = ag.rec[et];
    }
    v.note("a top entry without a gather record");
    std::vector<ResidRec> xr(x.xv.size() + 1, ResidRec{-1, 0, 0});
    for (size_t j = 0; j < x.xv.size(); j++) xr[j] = rg.rec[x.xv[j]];
    if (v.ok) {
      CXK_TRY(ctx->fx_xg.upload(xg));
      CXK_TRY(ctx->fx_xr.upload(xr));
      CXK_TRY(ctx->fx_done.alloc(64 * 16, true));  // 64 counters, 128 bytes apart
      ctx->fx_done_target = 0;
    }
  }
  if (!v.ok) return v.refuse(sw, "whole-tree launch");
  ft.xreg.resize(ft.xreg.size() + kPullPad, 0);
  ft.xsrc.resize(ft.xsrc.size() + kPullPad * kFusedExtraMax, -1ll);
  ft.rsrc.resize(ft.rsrc.size() + 64 * kFusedExtraMax, -1ll);
  ft.pub.resize(ft.pub.size() + 64, (int)u.slots);
  // hand-off slots: every slot with a producer starts as the sentinel in BOTH sets, the rest 0.0
  const double sent = [] {
    double d;
    const unsigned long long bits = kFusedSentinel;
    memcpy(&d, &bits, sizeof(d));
    return d;
  }();
  // (forward-value slots three times over: right-hand sides 1 and 2 of a launch with three, kFusedTriple)
  const size_t hs = us + 3 * ubs + 8;
  ctx->fx_updb_base = (long long)us;
  ctx->fx_fwd_stride = (long long)ubs;
  ctx->fx_hand_init.assign(2 * hs, 0.0);
  for (size_t t = 0; t + 64 < ft.pub.size(); t++) {
    const int d = ft.pub[t];
    if (d != (int)u.slots && d != (int)us + u.slotsb) {
      ctx->fx_hand_init[d] = ctx->fx_hand_init[hs + d] = sent;
      if ((size_t)d >= us)
        for (size_t q = 1; q < 3; q++) ctx->fx_hand_init[d + q * ubs] = ctx->fx_hand_init[hs + d + q * ubs] = sent;
    }
  }
  if (!split && !sharded && !sw.fused_level_order) DealOverXcds(ctx, pos_of, &ft);
  if (ft.img_stride > 0) {
    const double consts[2] = {0.0, 1.0};  // (what the images' entries that do not exist point at)
    CXK_TRY(hipMemcpy(ctx->G.p + ctx->G.n - 2, consts, sizeof(consts), hipMemcpyHostToDevice));
  }
  CXK_TRY(ctx->fx_img.upload(ft.img));
  CXK_TRY(ctx->fx_rec.upload(ft.recs));
  CXK_TRY(ctx->fx_xreg.upload(ft.xreg));
  CXK_TRY(ctx->fx_xsrc.upload(ft.xsrc));
  CXK_TRY(ctx->fx_rsrc.upload(ft.rsrc));
  CXK_TRY(ctx->fx_pub.upload(ft.pub));
  CXK_TRY(ctx->fx_hand.upload(ctx->fx_hand_init));
  CXK_TRY(ctx->fx_ysig.upload(std::vector<double>(6 * (size_t)N, sent)));  // two sets x three right-hand sides
  CXK_TRY(ctx->y3.alloc(3 * (size_t)N, true));
  ctx->fused_tgen = 0;
  ctx->y3_valid = false;
  if (!ctx->fx_flag) {
    CXK_TRY(hipHostMalloc(reinterpret_cast<void**>(&ctx->fx_flag), 64, hipHostMallocDefault));
    *ctx->fx_flag = 0.0;
  }
  ctx->fused_sa = sa;
  ctx->fused_sb = sb;
  ctx->fused_gen = 0;
  ctx->fused_tree = true;
  ctx->fused_split = split;
  ctx->fused_shard = sharded;
  ctx->fused_up = cnt_up;
  // (solve-only sweeps of a sharded context keep the level kernels and their own small exchange)
  ctx->fused_sweep = !sharded && !sw.no_fused_sweep;
  if (sw.debug_levels)
    fprintf(stderr, "whole tree in %s: %d supernodes, shapes <%d,%d> <%d,%d>, %zu entries / %zu variables with further sources\n",
            sharded ? "two launches around the exchange (own subtrees up + pack, top + down)" : split ? "two launches (up, down)" : "one launch", cnt_all, sa >> 8, sa & 255, sb >> 8, sb & 255,
            ft.xreg.size() - kPullPad, ft.rsrc.size());
  return CXK_SUCCESS;
}

// ---- the top as one dense T x T factorization (single GPU, Cholesky): tables for
// tree_top_dense.  Rows = the variables of the top supernodes in elimination order.
// Used where the supernode-by-supernode kernels are weak: when the last levels hold a mid-size
// supernode (33..64 columns: otherwise a 256-thread workgroup with two barriers per column,
// 62 us for C2's 50-column root).  The dense range [dense_level, nlev) starts at such a level;
// for tops made of small supernodes (C4) the supernode-by-supernode top measured faster.
int PlanTopDense(cxk_context* ctx, const PlanSwitches& sw, const UpdateSlots& u) {
  const Layout& L = ctx->lay;
  const int K = ctx->md.K, N = ctx->md.N, nlev = ctx->nlev;
  const std::vector<int>& ns = ctx->t_ns;
  const std::vector<int>& nsep = ctx->t_nsep;
  const std::vector<int>& start = ctx->t_start;
  ctx->top_dense.on = false;
  ctx->dense_level = nlev;
  Verdict v;
  v.check(ctx->world <= 1 && !ctx->use_ldlt && !sw.no_top_dense, "sharded, LDLT or CXK_NO_TOP_DENSE");
  int dt = -1;
  if (v.ok) {
    int cols = 0, count = 0;
    bool clean = true;
    for (int l = nlev - 1; l >= 0 && clean; l--) {
      if (ctx->level_nh[l] != ctx->level_ptr[l + 1] - ctx->level_ptr[l]) break;  // a panel beyond LDS
      for (int pos = ctx->level_ptr[l]; pos < ctx->level_ptr[l + 1]; pos++) {
        cols += ns[ctx->level_sn[pos]];
        count++;
      }
      if (cols > kTopMaxCols || count > kTopMaxSn) break;
      if (ctx->level_big[l]) dt = l;
    }
  }
  v.check(dt >= 0, "no level of mid-size supernodes among the top levels that fit");
  std::vector<int> tsn;
  int T = 0;
  if (v.ok) {
    for (int pos = ctx->level_ptr[dt]; pos < ctx->level_ptr[nlev]; pos++) tsn.push_back(ctx->level_sn[pos]);
    std::sort(tsn.begin(), tsn.end());
    for (int e : tsn) T += ns[e];
  }
  v.check(!tsn.empty() && (int)tsn.size() <= kTopMaxSn && T <= kTopMaxCols && T > 0, "too many supernodes or columns");
  if (!v.ok) return v.refuse(sw, "dense top");
  TopDenseArgs& a = ctx->top_dense.args;
  a.nt = (int)tsn.size();
  a.T = T;
  std::vector<int> is_top(K, -1), vrow(N, -1);
  int row = 0, base = 0;
  for (int k = 0; k < a.nt; k++) {
    const int e = tsn[k];
    is_top[e] = k;
    a.ns[k] = ns[e];
    a.nsep[k] = nsep[e];
    a.start[k] = start[e];
    a.row0[k] = row;
    a.base[k] = base;
    a.diag_off[k] = L.diag_off[e];
    a.offd_off[k] = L.offd_off[e];
    for (int i2 = 0; i2 < ns[e]; i2++) vrow[start[e] + i2] = row + i2;
    row += ns[e];
    base += ns[e] * ns[e] + ns[e] * nsep[e];
  }
  for (int k = 0; k < a.nt && v.ok; k++)  // separators of the top stay inside the top
    for (int x : L.separators[tsn[k]])
      if (vrow[x] < 0) v.ok = false;
  v.note("a separator outside the top");
  v.check(base <= kTopMaxCols * kTopMaxCols, "the panels exceed the dense image");
  if (!v.ok) return v.refuse(sw, "dense top");
  std::vector<int> off((size_t)T * T, -1);
  for (int k = 0; k < a.nt; k++) {
    const int e = tsn[k], n = ns[e];
    for (int jl = 0; jl < n; jl++) {
      const int j = a.row0[k] + jl;
      for (int rl = jl; rl < n; rl++) off[(size_t)(a.row0[k] + rl) * T + j] = a.base[k] + rl + jl * n;
      const IntList& sp = L.separators[e];
      for (int c = 0; c < (int)sp.size(); c++) off[(size_t)vrow[sp[c]] * T + j] = a.base[k] + n * n + jl + c * n;
    }
  }
  // Updates from below the top arrive through the supernodes' consumer-ordered slots; slots
  // fed from inside the top are never written in this mode (they hold 0.0).  Forward-solve
  // values use explicit fixed-width lists (the forward-only sweeps do write the inner slots).
  std::vector<int64_t> updb_off64(u.updb_off.begin(), u.updb_off.end());
  auto producer = [&](const std::vector<int64_t>& offs, int64_t q) {
    return (int)(std::upper_bound(offs.begin(), offs.end(), q) - offs.begin()) - 1;
  };
  int u_lds = 0, t_lds = 0;
  std::vector<int> rhs_src((size_t)T * kTopRhsSrc, u.slotsb + 1);  // slotsb + 1: never written, 0.0
  for (int k = 0; k < a.nt && v.ok; k++) {
    const int e = tsn[k];
    a.ubase[k] = (int)u.ubase[e];
    a.m[k] = u.m[e];
    a.tg_beg[k] = u.tg_ptr[e];
    a.ntg[k] = u.tg_ptr[e + 1] - u.tg_ptr[e];
    a.ubase_lds[k] = u_lds;
    a.tg_lds[k] = t_lds;
    u_lds += a.ntg[k] * a.m[k];
    t_lds += a.ntg[k];
    for (int i2 = 0; i2 < ns[e]; i2++) {
      int cnt2 = 0;
      for (int q : u.fs[start[e] + i2])
        if (is_top[producer(updb_off64, q)] < 0) {
          if (cnt2 == kTopRhsSrc) {
            v.ok = false;
            break;
          }
          rhs_src[(size_t)(a.row0[k] + i2) * kTopRhsSrc + cnt2++] = u.pubb_dst[q];
        }
    }
  }
  v.note("more forward-solve sources per row than the fixed-width lists hold");
  v.check(u_lds <= kTopMaxImage && t_lds <= kTopMaxImage, "the update slots exceed the dense image");
  if (!v.ok) return v.refuse(sw, "dense top");
  CXK_TRY(ctx->top_dense.off.upload(off));
  CXK_TRY(ctx->top_dense.pl_src.upload(rhs_src));
  a.top_off = ctx->top_dense.off.p;
  a.rhs_src = ctx->top_dense.pl_src.p;
  CXK_TRY(RaiseTopDenseLimits());
  ctx->top_dense.on = true;
  ctx->dense_level = dt;
  return CXK_SUCCESS;
}

// ---- level ranges below the top: merge consecutive levels into one launch when every
// connected piece of the forest restricted to them fits one workgroup (<= 8 supernodes per
// level: one wavefront each, and <= kRangeMaxRecs records for the LDS prefetch)
int PlanRanges(cxk_context* ctx) {
  const Layout& L = ctx->lay;
  const int K = ctx->md.K;
  ctx->ranges.clear();
  if (ctx->world > 1 || ctx->use_ldlt) return CXK_SUCCESS;
  const int top = ctx->top_level;
  std::vector<int> pos_of(K, -1);
  for (size_t pos = 0; pos < ctx->level_sn.size(); pos++) pos_of[ctx->level_sn[pos]] = (int)pos;
  std::vector<int> uf(K);
  auto find = [&](int x) {
    while (uf[x] != x) x = uf[x] = uf[uf[x]];
    return x;
  };
  // pieces[root] -> per level list of supernodes; returns false when a piece is too wide
  auto build = [&](int lo, int hi, std::vector<std::vector<std::vector<int>>>* out) {
    for (int e = 0; e < K; e++) uf[e] = e;
    auto in = [&](int e) { return ctx->t_ns[e] > 0 && pos_of[e] >= 0 && ctx->t_level[e] >= lo && ctx->t_level[e] < hi; };
    for (int e = 0; e < K; e++) {
      if (!in(e)) continue;
      for (int v : L.separators[e]) {
        const int a = L.var_to_sn[v];
        if (in(a)) uf[find(e)] = find(a);
      }
    }
    std::map<int, int> index;
    out->clear();
    for (int pos = ctx->level_ptr[lo]; pos < ctx->level_ptr[hi]; pos++) {  // level order keeps lists sorted
      const int e = ctx->level_sn[pos];
      const int r = find(e);
      auto it = index.find(r);
      if (it == index.end()) {
        it = index.emplace(r, (int)out->size()).first;
        out->emplace_back(hi - lo);
      }
      (*out)[it->second][ctx->t_level[e] - lo].push_back(e);
    }
    for (auto& piece : *out) {
      size_t total = 0;
      for (auto& lev : piece) {
        if (lev.size() > 8) return false;
        total += lev.size();
      }
      if (total > (size_t)kRangeMaxRecs) return false;
    }
    return true;
  };
  std::vector<SnRec> rr;
  int lo = 0;
  while (lo < top) {
    int hi = lo + 1;
    std::vector<std::vector<std::vector<int>>> pieces, trial;
    bool any_big = ctx->level_big[lo];
    if (!any_big)
      while (hi < top && !ctx->level_big[hi] && hi - lo < 8 && build(lo, hi + 1, &trial)) {
        pieces.swap(trial);
        hi++;
      }
    bool all_lean = !ctx->no_lean;
    for (int l = lo; l < hi; l++) all_lean = all_lean && ctx->level_lean[l];
    if (all_lean) {  // every level has its shape-specialised backward kernel: faster than the merged sweep
      lo = hi;
      continue;
    }
    if (hi - lo > 1) {
      cxk_context::SweepRange rg;
      rg.lo = lo;
      rg.hi = hi;
      rg.groups = (int)pieces.size();
      std::vector<int> tab;
      size_t widest = 1;
      for (auto& piece : pieces) {
        for (auto& lev : piece) {
          tab.push_back((int)rr.size());
          widest = std::max(widest, lev.size());
          for (int e : lev) rr.push_back(ctx->h_recs[pos_of[e]]);
        }
        tab.push_back((int)rr.size());
      }
      rg.waves = (int)widest;
      CXK_TRY(rg.wg_lev.upload(tab));
      ctx->ranges.push_back(std::move(rg));
    }
    lo = hi;
  }
  CXK_TRY(ctx->rec_r.upload(rr));
  return CXK_SUCCESS;
}

// ---- the per-supernode arrays and the device pointers of the level kernels (FactorPlan)
int UploadFactorPlan(cxk_context* ctx) {
  CXK_TRY(ctx->p_ns.upload(ctx->t_ns));
  CXK_TRY(ctx->p_nsep.upload(ctx->t_nsep));
  CXK_TRY(ctx->p_start.upload(ctx->t_start));
  CXK_TRY(ctx->p_diag.upload(ctx->lay.diag_off));
  CXK_TRY(ctx->p_offd.upload(ctx->lay.offd_off));
  FactorPlan& P = ctx->plan;
  P.rec = ctx->p_rec.p;
  P.ns = ctx->p_ns.p;
  P.nsep = ctx->p_nsep.p;
  P.start = ctx->p_start.p;
  P.diag_off = ctx->p_diag.p;
  P.offd_off = ctx->p_offd.p;
  P.upd_off = ctx->upd_off.p;
  P.updb_off = ctx->updb_off.p;
  P.tg_ptr = ctx->tg_ptr.p;
  P.tg_loc = ctx->tg_loc.p;
  P.tg_reg = ctx->tg_reg.p;
  P.tr_ptr = ctx->tr_ptr.p;
  P.tr_src = ctx->tr_src.p;
  P.fs_ptr = ctx->fs_ptr.p;
  P.fs_src = ctx->fs_src.p;
  P.upd = ctx->upd.p;
  P.pub_dst = ctx->pub_dst.p;
  P.pubb_dst = ctx->pubb_dst.p;
  P.updb = ctx->updb.p;
  P.bs_ptr = ctx->bs_ptr.p;
  P.bs_c = ctx->bs_c.p;
  P.bs_row = ctx->bs_row.p;
  return CXK_SUCCESS;
}

}  // namespace

// Every host-side planning decision of a context, once, at cxk_finalize.  Each stage uploads its
// own tables at its end.  Order dependencies:
//  - the gathers and the update slots come first: the fused assembly and the fused tree read the
//    gather records (the fused assembly uploads shrunk copies, as_rec2 / rs_rec2, next to the full
//    lists), the levels, the exchange, the fused tree and the dense top read the slots;
//  - the level records (PlanLevels) need the slots and the backward order; every later stage reads
//    the level lists, segments and records;
//  - the chain needs the top level; the backward pairs, the lean solve, the fused assembly and the
//    ranges need both; the fused tree's top positions read the exchange layout.
int BuildPlans(cxk_context* ctx) {
  const PlanSwitches sw;
  ctx->no_lean = sw.no_lean;
  ctx->no_ranges = sw.no_ranges;
  AsmGather gather;
  ResidGather resid;
  UpdateSlots slots;
  ExchangeLayout exchange;
  BackwardOrder backward;
  if (PlanAssemblyGather(ctx, &gather) != CXK_SUCCESS) return CXK_FAILURE;
  if (PlanResidualGather(ctx, &resid) != CXK_SUCCESS) return CXK_FAILURE;
  if (PlanCliqueVariables(ctx) != CXK_SUCCESS) return CXK_FAILURE;
  if (PlanUpdateSlots(ctx, &slots) != CXK_SUCCESS) return CXK_FAILURE;
  if (PlanExchange(ctx, slots, &exchange) != CXK_SUCCESS) return CXK_FAILURE;
  if (PlanBackwardOrder(ctx, &backward) != CXK_SUCCESS) return CXK_FAILURE;
  if (PlanLevels(ctx, sw, slots, backward) != CXK_SUCCESS) return CXK_FAILURE;
  PlanTopAndChain(ctx, sw);
  if (PlanBackPairs(ctx, sw) != CXK_SUCCESS) return CXK_FAILURE;
  PlanLeanSolve(ctx);
  if (PlanFusedAssembly(ctx, sw, gather, resid, slots) != CXK_SUCCESS) return CXK_FAILURE;
  if (PlanFusedTree(ctx, sw, gather, resid, slots, exchange) != CXK_SUCCESS) return CXK_FAILURE;
  if (PlanTopDense(ctx, sw, slots) != CXK_SUCCESS) return CXK_FAILURE;
  if (PlanRanges(ctx) != CXK_SUCCESS) return CXK_FAILURE;
  return UploadFactorPlan(ctx);
}

}  // namespace cxk_host
