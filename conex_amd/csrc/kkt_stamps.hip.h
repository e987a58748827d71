// In-kernel time stamps of the tree kernels (diagnostic builds only: -DCXK_DEBUG_STAMPS or
// -DCXK_CHAIN_STAMPS); values go to a buffer nothing else reads.  Without either flag the macros expand
// to nothing and no symbol is defined.  Read back by cxk_debug_stamps (kkt_tree_launch.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace cxk {

#ifdef CXK_DEBUG_STAMPS
// g_cxk_want (set by cxk_debug_select): 0 = single-level factor launches, 1 = merged level ranges
// (grid > 1), 2 = the one-workgroup top.  Wave 0 of workgroup 0 records stamp i of level l of the
// launch at g_cxk_stamp[8 l + i]; the backward stamps go to [64 + i].
__device__ long long g_cxk_stamp[96];
__device__ int g_cxk_sel, g_cxk_want, g_cxk_lvl;
#define CXK_STAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == 0 && g_cxk_sel == 1) g_cxk_stamp[8 * g_cxk_lvl + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#define CXK_STAMPB(i) do { if (blockIdx.x == 0 && threadIdx.x == 0 && g_cxk_sel == 2) g_cxk_stamp[64 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#define CXK_STAMP_SELECT(lb, mode) do { if (blockIdx.x == 0 && threadIdx.x == 0) { g_cxk_lvl = 0; const int kind = (lb) == 0 ? 0 : (gridDim.x > 1 ? 1 : 2); g_cxk_sel = (kind == g_cxk_want) ? ((mode) == 0 ? 1 : ((mode) == 2 ? 2 : 0)) : 0; } } while (0)
#define CXK_STAMP_LEVEL(l) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_cxk_lvl = (l); } while (0)
#else
#ifdef CXK_CHAIN_STAMPS  // only the chain kernel's register-held stamps (tree_chain_lean)
__device__ long long g_cxk_stamp[96];
#endif
#define CXK_STAMP(i) do { } while (0)
#define CXK_STAMPB(i) do { } while (0)
#define CXK_STAMP_SELECT(lb, mode) do { } while (0)
#define CXK_STAMP_LEVEL(l) do { } while (0)
#endif

}  // namespace cxk
