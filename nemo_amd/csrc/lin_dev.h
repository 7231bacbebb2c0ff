// lin_dev.h — what the kernels of the two lineage searches (k_lineage.hip: nemo_lineage_cuts; k_lgcuts.hip:
// nemo_lineage_group_cuts) share on the device: a set's key in device memory, a wave's prefix sum, a chunk's keys into
// LDS, the emission of a chunk's children, and the entry of a cut into the cuts' table (LinArgs: internal.h; the keys
// and the hash: lin_host.h).
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

// a chunk's n keys front[first .. first + n) into s_key, thread t key t.  No barrier: the caller's next one publishes them
__device__ __forceinline__ void lin_stage_keys(const uint64_t *front, uint32_t first, uint32_t n, uint64_t (*s_key)[2]) {
  const uint32_t tid = threadIdx.x;
  if (tid < n) {
    const lin::Key k = lin_load(front, first + tid);
    s_key[tid][0] = k.lo, s_key[tid][1] = k.hi;
  }
}

// The children of a chunk (its keys in s_key) that candidate position k adds: (set h) + {k} for every bit h of this
// lane's w.  A whole wave calls it, a lane per position (w = 0 past the last): one claim on the global cursor for the
// wave's children, which counts past the buffer's end; nothing is written there.
__device__ __forceinline__ void lin_emit(const LinArgs &l, const uint64_t (*s_key)[2], uint32_t k, uint64_t w) {
  uint32_t total;
  const uint32_t pre = lin_wave_scan((uint32_t)__popcll(w), &total);
  if (!total) return;
  unsigned long long at = 0;
  if (lane_id() == 0u) at = atomicAdd(l.ctr + 1, (unsigned long long)total);
  at = (unsigned long long)__shfl((unsigned long long)at, 0) + pre;
  for (; w; w &= w - 1ull, at++) {
    if (at >= l.kids_cap) break;  // counted, not written
    const int h = __ffsll((long long)w) - 1;
    lin_store(l.kids, at, lin::key_insert(lin::Key{s_key[h][0], s_key[h][1]}, k));
  }
}

// cut i (its key is in a.cuts) into the cuts' table: the cuts are distinct sets, so a taken slot is another's
__device__ __forceinline__ void lin_cut_insert(const LinArgs &a, uint32_t i, const lin::Key &k) {
  uint64_t h = lin::first_slot(k, a.cslots);
  while (atomicCAS(&a.ctab[h], 0u, i + 1u) != 0u) h = lin::next_slot(h, a.cslots);  // ends: at most half of the slots are taken
}

}  // namespace nemo
