// cut_dev.h — what the sweep kernels of the two searches of sets of size <= 3 over one graph share on the device
// (k_cuts.hip: k_cut_lds, k_cut_glob; k_repair.hip: k_repair_lds, k_repair_glob): the persistent loop over a round's
// chunks of 64 hypotheses.  A round's hypotheses are the sets of 1, 2 or 3 live candidates in colex rank order
// (cut_host.h), so a workgroup makes a chunk's seeds from the chunk's index alone.  The two modes are monotone duals:
// a cut search starts a chunk's dead words from zeros and a hypothesis sets its column on the nodes it names; a repair
// search starts them from the absent bitmap (all 64 columns set on an absent node), a hypothesis clears its column
// on the nodes it restores, and the result word is the complement of the lost word.  The image, the zeroing, the
// sweep and the lost word are ko_sweep.h's; round 3's pair test is cut_host.h's.
#pragma once
#include "cut_host.h"
#include "device.h"
#include "internal.h"
#include "ko_sweep.h"

namespace nemo {

// dead[v] = absent(v) ? ~0 : 0 where ko_zero_dead writes zeros: the same whole 16-byte pairs, the same fence and
// barrier behind them.  A pair's two nodes 2 i and 2 i + 1 lie in one word of the bitmap; the bits past V are 0, so
// an odd V's padding word stays 0.  The caller's last reads of the words lie behind a barrier, and so does the
// staging of the bitmap.  All 256 threads.
template <bool LDS>
__device__ __forceinline__ void repair_fill(const KoImg<LDS> &g, const uint64_t *absent) {
  uint4 *z = reinterpret_cast<uint4 *>(g.dead);
  const uint32_t pairs = (g.V + 1u) / 2u;
  for (uint32_t i = threadIdx.x; i < pairs; i += KO_BLOCK) {
    const uint32_t v = 2u * i;
    const uint32_t two = (uint32_t)(absent[v >> 6] >> (v & 63u)) & 3u;
    const uint32_t lo = (two & 1u) ? ~0u : 0u, hi = (two & 2u) ? ~0u : 0u;
    z[i] = make_uint4(lo, lo, hi, hi);
  }
  if (!LDS) __threadfence_block();
  __syncthreads();
}

// a hypothesis' column `bit` on node v: set by a cut, cleared by a repair (hypotheses of one chunk share nodes: atomic)
template <bool REPAIR>
__device__ __forceinline__ void cut_seed(unsigned long long *d64, uint32_t v, unsigned long long bit) {
  if constexpr (REPAIR) atomicAnd(&d64[v], ~bit);
  else atomicOr(&d64[v], bit);
}

// All chunks ci = blockIdx.x, += gridDim.x of the round on a graph whose image (REPAIR: and bitmap `absent`) is in
// place.  SIZE: the round, a template parameter, so no unrank path diverges; REPAIR has a round 0: one chunk, column 0
// restores nothing and column 1 every candidate a.cand[0 .. n_cand).  All 256 threads.
template <bool LDS, uint32_t SIZE, bool REPAIR>
__device__ __forceinline__ void cut_loop(const CutArgs &a, const KoImg<LDS> &g, const uint64_t *absent, uint32_t n_cand) {
  static_assert(REPAIR || SIZE >= 1u, "only the repair search has a round 0");
  __shared__ uint64_t s_and[KO_BLOCK / 64];
  const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  unsigned long long *d64 = reinterpret_cast<unsigned long long *>(g.dead);
  for (uint32_t ci = blockIdx.x; ci < a.n_chunks; ci += gridDim.x) {
    // the previous chunk's words go (its last reads lie behind the barrier that ends the loop body)
    if constexpr (REPAIR) repair_fill<LDS>(g, absent);
    else ko_zero_dead<LDS>(g);
    const uint32_t first = ci * KO_CHUNK, n = min(KO_CHUNK, a.n_hyp - first);
    bool sub = false;  // round 3: one of the set's pairs is a cut / a repair already
    if constexpr (SIZE == 0u) {
      // column 0 restores nothing; column 1 restores every candidate (distinct nodes; atomic as the other rounds')
      for (uint32_t k = tid; k < n_cand; k += KO_BLOCK) {
        const uint32_t v = a.cand[k];
        if (v < g.V) cut_seed<REPAIR>(d64, v, 2ull);
      }
    } else if (tid < n) {
      // seeds: lane t's hypothesis is the set of rank first + t
      const uint64_t h = (uint64_t)first + tid;
      const unsigned long long bit = 1ull << tid;
      const cuts::Pos p = cuts::unrank<(SIZE ? SIZE : 1u)>(h);
      const uint32_t va = a.lnode[p.a], vb = SIZE >= 2u ? a.lnode[p.b] : g.V, vc = SIZE >= 3u ? a.lnode[p.c] : g.V;
      if (va < g.V) cut_seed<REPAIR>(d64, va, bit);
      if constexpr (SIZE >= 2u)
        if (vb < g.V) cut_seed<REPAIR>(d64, vb, bit);
      if constexpr (SIZE >= 3u)
        if (vc < g.V) cut_seed<REPAIR>(d64, vc, bit);
      if constexpr (SIZE == 3u) sub = cuts::has_cut_pair(a.pairs, p);  // round 2's words, read while the sweep runs
    }
    if (!LDS) __threadfence_block();
    __syncthreads();
    ko_sweep<LDS>(g);
    // lost: every root dead, per bit column; a repair's word is "some root alive".  Every thread holds the lost
    // word; wave 0, whose lanes hold the chunk's `sub`, finishes.  (s_and is written next behind the next chunk's
    // barriers.)
    uint64_t w = ko_lost_word<LDS>(g, n, s_and);
    if (wave == 0) {
      if constexpr (REPAIR) w = ~w & (n == KO_CHUNK ? ~0ull : (1ull << n) - 1ull);
      if constexpr (SIZE == 3u) w &= ~__ballot(sub);
      if (lane == 0) a.words[ci] = w;
    }
  }
}

}  // namespace nemo
