// lin_dev.h — what the kernels of the two lineage searches (k_lineage.hip: nemo_lineage_cuts; k_lgcuts.hip:
// nemo_lineage_group_cuts) share on the device: a set's key in device memory, a wave's prefix sum, and the entry of a
// cut into the cuts' table (LinArgs: internal.h; the keys and the hash: lin_host.h).
#pragma once
#include "device.h"
#include "internal.h"
#include "lin_host.h"

namespace nemo {

__device__ __forceinline__ lin::Key lin_load(const uint64_t *keys, uint64_t i) {
  const ulonglong2 k = *reinterpret_cast<const ulonglong2 *>(keys + 2ull * i);
  return lin::Key{k.x, k.y};
}
__device__ __forceinline__ void lin_store(uint64_t *keys, uint64_t i, const lin::Key &k) {
  *reinterpret_cast<ulonglong2 *>(keys + 2ull * i) = make_ulonglong2(k.lo, k.hi);
}

// the wave's exclusive prefix of n and, in every lane, the wave's sum
__device__ __forceinline__ uint32_t lin_wave_scan(uint32_t n, uint32_t *total) {
  const uint32_t lane = lane_id();
  uint32_t incl = n;
#pragma unroll
  for (int dd = 1; dd < 64; dd <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)incl, dd);
    if ((int)lane >= dd) incl += y;
  }
  *total = (uint32_t)__shfl((int)incl, 63);
  return incl - n;
}

// cut i (its key is in a.cuts) into the cuts' table: the cuts are distinct sets, so a taken slot is another's
__device__ __forceinline__ void lin_cut_insert(const LinArgs &a, uint32_t i, const lin::Key &k) {
  uint64_t h = lin::first_slot(k, a.cslots);
  while (atomicCAS(&a.ctab[h], 0u, i + 1u) != 0u) h = lin::next_slot(h, a.cslots);  // ends: at most half of the slots are taken
}

}  // namespace nemo
