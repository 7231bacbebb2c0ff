// hit_list.h — a graph's hit list as k_lcuts.hip, k_gcuts.hip, k_witness.hip and k_lgcuts.hip keep it: the graph's nodes grouped by a row id
// (k_lc_*: the live position of the node's label; k_gc_*: the distinct label itself), k1 rows, u32 entries:
// [0 .. k1] the rows' offsets, then the rows' nodes.  The first `cap` entries live in LDS behind the image, the
// others in the workgroup's region (lcut_host.h: list_entries, region_words).
#pragma once
#include "ko_sweep.h"

namespace nemo {

struct LcList {
  uint32_t *head, *spill;
  uint32_t cap;
  __device__ __forceinline__ uint32_t get(uint32_t i) const { return i < cap ? head[i] : spill[i - cap]; }
  __device__ __forceinline__ void set(uint32_t i, uint32_t x) const {
    if (i < cap) head[i] = x;
    else spill[i - cap] = x;
  }
  __device__ __forceinline__ uint32_t add(uint32_t i) const { return i < cap ? atomicAdd(&head[i], 1u) : atomicAdd(&spill[i - cap], 1u); }
  // row p of a built list is entries [lo(p), hi(p)) behind the k1 + 1 offsets
  __device__ __forceinline__ uint32_t lo(uint32_t p) const { return p ? get(p - 1u) : 0u; }
  __device__ __forceinline__ uint32_t hi(uint32_t p) const { return get(p); }
};

// Groups the V nodes of a staged graph by row: count, scan, scatter.  row_of(v) is node v's row, below k1, or
// UINT32_MAX for a node that belongs to none; it is called twice per node and must give the same answer.  The
// caller's last reads of the previous list lie behind a barrier; the staging of the image that row_of may read
// ends at the first barrier here.  Ends behind a barrier: row p is entries [lo(p), hi(p)).  All 256 threads.
template <class F>
__device__ __forceinline__ void hit_list_build(const LcList &ls, uint32_t V, uint32_t k1, F &&row_of) {
  const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  for (uint32_t i = tid; i <= k1; i += KO_BLOCK) ls.set(i, 0u);
  __threadfence_block();  // the entries in the region
  __syncthreads();        // ... and the image: the rule bits and rows are read below
  for (uint32_t v = tid; v < V; v += KO_BLOCK) {  // count per row
    const uint32_t r = row_of(v);
    if (r != 0xFFFFFFFFu) ls.add(r);
  }
  __threadfence_block();
  __syncthreads();
  if (wave == 0u) {  // exclusive scan of the k1 + 1 counts (the last one is 0: it becomes the total)
    uint32_t carry = 0u;
    for (uint32_t base = 0; base <= k1; base += 64u) {
      const uint32_t i = base + lane;
      const uint32_t x = i <= k1 ? ls.get(i) : 0u;
      uint32_t incl = x;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)incl, d);
        if ((int)lane >= d) incl += y;
      }
      if (i <= k1) ls.set(i, carry + incl - x);
      carry += (uint32_t)__shfl((int)incl, 63);
    }
  }
  __threadfence_block();
  __syncthreads();
  for (uint32_t v = tid; v < V; v += KO_BLOCK) {  // scatter: a row's cursor ends at the next row's start
    const uint32_t r = row_of(v);
    if (r != 0xFFFFFFFFu) ls.set(k1 + 1u + ls.add(r), v);
  }
  __threadfence_block();
  __syncthreads();  // row p is now entries [p ? off[p - 1] : 0, off[p]) behind the offsets
}

}  // namespace nemo
