// ko_sweep.h — what the knock-out kernels (k_knock.hip) and the cut-set kernels (k_cuts.hip) share: a raw
// provenance graph as the sweep reads it, k_ko_lds's LDS image of it, and the level sweep itself, which does not
// know where the seeds of its 64 hypotheses came from (DESIGN.md §Knock-out, §Minimal cut sets).
#pragma once
#include <type_traits>

#include "device.h"
#include "knock_host.h"

namespace nemo {

#define KO_BLOCK 256
#define KO_Q 4      // 16-byte chunks of node words per thread and round: 16 consecutive nodes
#define KO_HUB 32u  // a row of more children than this is folded by the whole wave

// The graph as the sweep reads it: u16 arrays in LDS (k_ko_lds, k_cut_lds) or the u32 CSR in device memory
// (k_ko_glob, k_cut_glob).
template <bool LDS>
struct KoImg {
  using idx = typename std::conditional<LDS, uint16_t, uint32_t>::type;
  const idx *fp, *fc, *topo, *lvl;
  const uint64_t *rule;  // LDS: a bit per node
  const uint32_t *word;  // else the node words
  uint64_t *dead;        // [V] (whole 16-byte pairs)
  uint32_t V, L;
  __device__ __forceinline__ bool is_rule_node(uint32_t v) const {
    return LDS ? ((rule[v >> 6] >> (v & 63u)) & 1ull) != 0ull : is_rule(word[v]);
  }
};

// The LDS image of graph gv carved from dyn (knock_lds_bytes) and filled, all 256 threads: dead words (not
// zeroed), forward rows, Kahn order and level offsets as u16, a rule bit per node.  No barrier at the end.
__device__ __forceinline__ KoImg<true> ko_stage_image(const GraphView &gv, uint8_t *dyn) {
  const uint32_t tid = threadIdx.x, lane = lane_id();
  const uint32_t V = gv.V, E = gv.E, L = gv.nlev;
  uint8_t *p = dyn;
  uint64_t *dead = reinterpret_cast<uint64_t *>(p);
  p += knock::ko_align(8u * V);
  uint16_t *fp = reinterpret_cast<uint16_t *>(p);
  p += knock::ko_align(2u * (V + 1u));
  uint16_t *fc = reinterpret_cast<uint16_t *>(p);
  p += knock::ko_align(2u * E);
  uint16_t *topo = reinterpret_cast<uint16_t *>(p);
  p += knock::ko_align(2u * V);
  uint16_t *lvl = reinterpret_cast<uint16_t *>(p);
  p += knock::ko_align(2u * (L + 1u));
  uint64_t *rule = reinterpret_cast<uint64_t *>(p);
  // the rule bits from the node words: every load of a round before the first ballot
  for (uint32_t base = 0; base < V; base += KO_Q * KO_BLOCK) {
    uint32_t w[KO_Q];
#pragma unroll
    for (int q = 0; q < KO_Q; q++) w[q] = gv.word[min(base + q * KO_BLOCK + tid, V - 1u)];
#pragma unroll
    for (int q = 0; q < KO_Q; q++) {
      const uint32_t v = base + q * KO_BLOCK + tid;
      const uint64_t m = __ballot(v < V && is_rule(w[q]));
      if (lane == 0 && v < V) rule[v >> 6] = m;
    }
  }
  const StageDesc d[4] = {{gv.fp, fp, V + 1u, ST_U16}, {gv.fc, fc, E, ST_U16}, {gv.topo, topo, V, ST_U16},
                          {gv.lvl, lvl, L + 1u, ST_U16}};
  stage_lds<4, KO_BLOCK>(d);
  KoImg<true> g;
  g.fp = fp, g.fc = fc, g.topo = topo, g.lvl = lvl, g.rule = rule, g.word = nullptr, g.dead = dead, g.V = V, g.L = L;
  return g;
}

// The sweep over a graph whose dead words hold the seeds (behind a barrier): levels nlev-1 .. 0; a node's
// children lie on strictly deeper levels, so their words are final.  Pull form: no atomics, one barrier per
// level, the last one behind level 0.  All 256 threads.
template <bool LDS>
__device__ __forceinline__ void ko_sweep(const KoImg<LDS> &g) {
  const uint32_t tid = threadIdx.x, lane = lane_id();
  uint64_t *dead = g.dead;
  for (int l = (int)g.L - 1; l >= 0; l--) {
    const uint32_t lo = g.lvl[l], hi = g.lvl[l + 1];
    for (uint32_t base = lo; base < hi; base += KO_BLOCK) {
      const uint32_t i = base + tid;
      const bool act = i < hi;
      const uint32_t v = act ? (uint32_t)g.topo[i] : 0u;
      const uint32_t b = act ? (uint32_t)g.fp[v] : 0u, e = act ? (uint32_t)g.fp[v + 1u] : 0u;
      const bool rule = act && g.is_rule_node(v);
      const bool hub = e - b > KO_HUB;
      uint64_t acc = (rule || e == b) ? 0ull : ~0ull;
      if (!hub)
        for (uint32_t j = b; j < e; j++) {
          const uint64_t w = dead[g.fc[j]];
          acc = rule ? acc | w : acc & w;
        }
      for (uint64_t hm = __ballot(hub); hm; hm &= hm - 1ull) {  // wave-uniform: one long row at a time
        const int src = __ffsll((long long)hm) - 1;
        const uint32_t hb = (uint32_t)__shfl((int)b, src), he = (uint32_t)__shfl((int)e, src);
        const bool hr = __shfl((int)rule, src) != 0;
        uint64_t part = hr ? 0ull : ~0ull;
        for (uint32_t j = hb + lane; j < he; j += 64u) {
          const uint64_t w = dead[g.fc[j]];
          part = hr ? part | w : part & w;
        }
#pragma unroll
        for (int dd = 32; dd >= 1; dd >>= 1) {
          const uint64_t y = (uint64_t)__shfl_xor((unsigned long long)part, dd);
          part = hr ? part | y : part & y;
        }
        if ((int)lane == src) acc = part;
      }
      if (act) dead[v] |= acc;  // the seed stays
    }
    if (!LDS) __threadfence_block();  // the level's words in device memory before the next level reads them
    __syncthreads();
  }
}

}  // namespace nemo
