// The time-out mark that the collectives of a sharded context carry (device functions only).
#pragma once
#include <hip/hip_runtime.h>

namespace cxk {

// The time-out mark of a sharded context's collectives behind a whole-tree factor launch (tag: that launch's).  A
// wait of the launch that ran out leaves fail[1] = tag and the pinned host word raised (tree_fused.hip; a failed
// pivot of the launch leaves fail[1] = tag alone).  The solve exchange and the step reductions carry 1.0 for it in
// one extra summed slot, and every rank that receives a mark > 0 records it as a failed factorization (fail[0])
// and a time-out of that launch (fail[2] = tag).  ResolveShardTimeout reads it.
__device__ __forceinline__ double ShardMark(const int* fail, int tag, const double* host_flag) {
  return tag != 0 && fail[1] == tag && __hip_atomic_load(host_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0.0
             ? 1.0
             : 0.0;
}
__device__ __forceinline__ void ShardMarkSeen(double mark, int* fail, int tag) {
  if (mark > 0.0 && tag != 0) {
    fail[0] = 1;
    fail[2] = tag;
  }
}

}  // namespace cxk
