// blame_down.h — the top-down blame pass of the lineage repair search, shared by both tiers of k_lrepair.hip
// (nemo_lineage_repair_sets / nemo_lineage_repairs; DESIGN.md §Lineage repair search): the dual of wit_down.h's need
// pass, with the roles of the kinds exchanged.  A blocker proves that every root is dead: a blamed rule blames its
// first dead child, a blamed goal every child, and a blamed node that is itself removed blames nothing further.  The
// words are read and ORed as wit_down.h's need words are.
#pragma once
#include "device.h"
#include "ko_sweep.h"
#include "wit_down.h"

namespace nemo {

// The top-down pass over a swept chunk (behind ko_sweep's last barrier and the lost word's): the blame words zeroed,
// the roots' set to `lost` (only a lost hypothesis has a blocker), then levels 0 .. L - 1, a thread per node.  A node's
// parents lie on strictly higher levels, so its word is final when its level is reached.  removed[v] holds the bits h
// under which v is in F_h (the chunk's seeds, before the sweep): those bits are dropped before v blames.  A row of
// more than KO_HUB children is taken by the whole wave: a goal's is a strided OR; a rule's goes in steps of 64
// children, `rem` carrying the bits under which every earlier child is alive and a wave scan of AND over the step's
// complemented dead words giving the same within the step.  Every blamed node is dead under its bits.  Ends behind a
// barrier.  All 256 threads, under a workgroup-uniform condition.
template <bool LDS>
__device__ __forceinline__ void blame_down(const KoImg<LDS> &g, uint64_t *blame, const uint64_t *removed, uint64_t lost) {
  const uint32_t tid = threadIdx.x, lane = lane_id();
  const uint64_t *dead = g.dead;
  {
    uint4 *z = reinterpret_cast<uint4 *>(blame);
    const uint32_t pairs = (g.V + 1u) / 2u;
    for (uint32_t i = tid; i < pairs; i += KO_BLOCK) z[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  if (!LDS) __threadfence_block();
  __syncthreads();
  const uint32_t n_roots = g.L ? (uint32_t)g.lvl[1] : 0u;
  if (lost)
    for (uint32_t i = tid; i < n_roots; i += KO_BLOCK) wit_or(&blame[g.topo[i]], lost);
  if (!LDS) __threadfence_block();
  __syncthreads();
  for (uint32_t l = 0; l < g.L; l++) {
    const uint32_t lo = g.lvl[l], hi = g.lvl[l + 1];
    for (uint32_t base = lo; base < hi; base += KO_BLOCK) {
      const uint32_t i = base + tid;
      const bool act = i < hi;
      const uint32_t v = act ? (uint32_t)g.topo[i] : 0u;
      const uint32_t b = act ? (uint32_t)g.fp[v] : 0u, e = act ? (uint32_t)g.fp[v + 1u] : 0u;
      const bool rule = act && g.is_rule_node(v);
      uint64_t nv = act ? wit_need<LDS>(&blame[v]) : 0ull;
      if (nv) nv &= ~wit_need<LDS>(&removed[v]);  // the stop rule
      const bool work = nv != 0ull && e > b;
      const bool hub = work && e - b > KO_HUB;
      if (work && !hub) {
        if (!rule) {
          for (uint32_t j = b; j < e; j++) wit_or(&blame[g.fc[j]], nv);
        } else {
          uint64_t rem = nv;
          for (uint32_t j = b; j < e && rem; j++) {
            const uint32_t c = g.fc[j];
            const uint64_t pick = rem & dead[c];
            if (pick) wit_or(&blame[c], pick);
            rem &= ~pick;
          }
        }
      }
      for (uint64_t hm = __ballot(hub); hm; hm &= hm - 1ull) {  // wave-uniform: one long row at a time
        const int src = __ffsll((long long)hm) - 1;
        const uint32_t hb = (uint32_t)__shfl((int)b, src), he = (uint32_t)__shfl((int)e, src);
        const bool hr = __shfl((int)rule, src) != 0;
        const uint64_t hn = (uint64_t)__shfl((unsigned long long)nv, src);
        if (!hr) {
          for (uint32_t j = hb + lane; j < he; j += 64u) wit_or(&blame[g.fc[j]], hn);
          continue;
        }
        uint64_t rem = hn;  // the same in every lane
        for (uint32_t jb = hb; jb < he && rem; jb += 64u) {
          const uint32_t j = jb + lane;
          const bool in = j < he;
          const uint32_t c = in ? (uint32_t)g.fc[j] : 0u;
          const uint64_t a = in ? ~dead[c] : ~0ull;  // alive; past the row's end: never picked, rem unchanged
          uint64_t incl = a;  // AND of the alive words of lanes 0 .. lane
#pragma unroll
          for (int dd = 1; dd < 64; dd <<= 1) {
            const uint64_t y = (uint64_t)__shfl_up((unsigned long long)incl, dd);
            if ((int)lane >= dd) incl &= y;
          }
          uint64_t pre = (uint64_t)__shfl_up((unsigned long long)incl, 1);  // ... of lanes 0 .. lane - 1
          if (lane == 0u) pre = ~0ull;
          const uint64_t pick = rem & pre & ~a;
          if (in && pick) wit_or(&blame[c], pick);
          rem &= (uint64_t)__shfl((unsigned long long)incl, 63);
        }
      }
    }
    if (!LDS) __threadfence_block();  // the level's ORs in device memory before the next level reads them
    __syncthreads();
  }
}

}  // namespace nemo
