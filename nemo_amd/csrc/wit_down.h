// wit_down.h — the top-down need pass of the surviving derivations, shared by k_witness.hip (nemo_witness_sets /
// nemo_witness_labels), k_lineage.hip (nemo_lineage_cuts) and k_lgcuts.hip (nemo_lineage_group_cuts), in the manner of ko_sweep.h and diff_walk.h: how a need
// word is read and ORed on either tier, and the pass itself over a swept chunk (DESIGN.md §Surviving derivations).
#pragma once
#include "device.h"
#include "ko_sweep.h"

namespace nemo {

// A need word as the pass and the epilogue read it.  The words are written by atomic ORs only (behind their
// zeroing); in device memory those are done in L2, so the read goes there too.
template <bool LDS>
__device__ __forceinline__ uint64_t wit_need(const uint64_t *p) {
  if (LDS) return *p;
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void wit_or(uint64_t *p, uint64_t bits) { atomicOr(reinterpret_cast<unsigned long long *>(p), bits); }

// The top-down pass over a swept chunk of n hypotheses (behind ko_sweep's last barrier): the need words zeroed, the
// roots' set to ~dead within the chunk's n bits, then levels 0 .. L - 1, a thread per node.  A node's parents lie on
// strictly higher levels, so its word is final when its level is reached.  A row of more than KO_HUB children is
// taken by the whole wave: a rule's is a strided OR; a goal's goes in steps of 64 children, `rem` carrying the bits
// under which every earlier child is dead and a wave scan of AND over the step's dead words giving the same within
// the step.  Ends behind a barrier.  All 256 threads.
template <bool LDS>
__device__ __forceinline__ void wit_down(const KoImg<LDS> &g, uint64_t *need, uint32_t n, bool all) {
  const uint32_t tid = threadIdx.x, lane = lane_id();
  const uint64_t *dead = g.dead;
  {
    uint4 *z = reinterpret_cast<uint4 *>(need);
    const uint32_t pairs = (g.V + 1u) / 2u;
    for (uint32_t i = tid; i < pairs; i += KO_BLOCK) z[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  if (!LDS) __threadfence_block();
  __syncthreads();
  const uint64_t tail = n == KO_CHUNK ? ~0ull : (1ull << n) - 1ull;
  const uint32_t n_roots = g.L ? (uint32_t)g.lvl[1] : 0u;
  for (uint32_t i = tid; i < n_roots; i += KO_BLOCK) {
    const uint32_t v = g.topo[i];
    const uint64_t w = ~dead[v] & tail;
    if (w) wit_or(&need[v], w);
  }
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
      const uint64_t nv = act ? wit_need<LDS>(&need[v]) : 0ull;
      const bool work = nv != 0ull && e > b;
      const bool hub = work && e - b > KO_HUB;
      if (work && !hub) {
        if (rule) {
          for (uint32_t j = b; j < e; j++) wit_or(&need[g.fc[j]], nv);
        } else {
          uint64_t rem = nv;
          for (uint32_t j = b; j < e && rem; j++) {
            const uint32_t c = g.fc[j];
            const uint64_t pick = rem & ~dead[c];
            if (pick) wit_or(&need[c], pick);
            if (!all) rem &= ~pick;
          }
        }
      }
      for (uint64_t hm = __ballot(hub); hm; hm &= hm - 1ull) {  // wave-uniform: one long row at a time
        const int src = __ffsll((long long)hm) - 1;
        const uint32_t hb = (uint32_t)__shfl((int)b, src), he = (uint32_t)__shfl((int)e, src);
        const bool hr = __shfl((int)rule, src) != 0;
        const uint64_t hn = (uint64_t)__shfl((unsigned long long)nv, src);
        if (hr) {
          for (uint32_t j = hb + lane; j < he; j += 64u) wit_or(&need[g.fc[j]], hn);
          continue;
        }
        uint64_t rem = hn;  // the same in every lane
        for (uint32_t jb = hb; jb < he && rem; jb += 64u) {
          const uint32_t j = jb + lane;
          const bool in = j < he;
          const uint32_t c = in ? (uint32_t)g.fc[j] : 0u;
          const uint64_t d = in ? dead[c] : ~0ull;
          uint64_t incl = d;  // AND of the dead words of lanes 0 .. lane
#pragma unroll
          for (int dd = 1; dd < 64; dd <<= 1) {
            const uint64_t y = (uint64_t)__shfl_up((unsigned long long)incl, dd);
            if ((int)lane >= dd) incl &= y;
          }
          uint64_t pre = (uint64_t)__shfl_up((unsigned long long)incl, 1);  // ... of lanes 0 .. lane - 1
          if (lane == 0u) pre = ~0ull;
          const uint64_t pick = all ? rem & ~d : rem & pre & ~d;
          if (in && pick) wit_or(&need[c], pick);
          if (!all) rem &= (uint64_t)__shfl((unsigned long long)incl, 63);
        }
      }
    }
    if (!LDS) __threadfence_block();  // the level's ORs in device memory before the next level reads them
    __syncthreads();
  }
}

}  // namespace nemo
