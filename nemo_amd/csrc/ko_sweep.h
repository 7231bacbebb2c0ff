// ko_sweep.h — what the knock-out family's kernels (k_knock.hip, k_cuts.hip, k_klabel.hip, k_lcuts.hip, k_gcuts.hip) share: a raw
// provenance graph as the sweep reads it, its LDS image and its global-tier form, the zeroing of the dead words, the
// level sweep itself, which does not know where the seeds of its 64 hypotheses came from, the "lost" word of a swept
// chunk, the count of a wave's bit columns, and on the host side the residency query and the dispatch on a round's
// size (DESIGN.md §Knock-out, §Minimal cut sets, §Knock-out by label, §Minimal cut sets by label).
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

// The global tier's image: the CSR in device memory as it lies, the dead words at `dead` (dead_words(V) of them).
// Pointers only: no load, no store, no barrier.
__device__ __forceinline__ KoImg<false> ko_glob_image(const GraphView &gv, uint64_t *dead) {
  KoImg<false> g;
  g.fp = gv.fp, g.fc = gv.fc, g.topo = gv.topo, g.lvl = gv.lvl, g.rule = nullptr, g.word = gv.word, g.dead = dead;
  g.V = gv.V, g.L = gv.nlev;
  return g;
}

// The image of either tier by tag: the LDS tier stages it into dyn (no barrier at the end), the global tier points
// at the CSR and keeps the dead words at the start of the workgroup's region reg.
__device__ __forceinline__ KoImg<true> ko_image(std::true_type, const GraphView &gv, uint8_t *dyn, uint64_t *) {
  return ko_stage_image(gv, dyn);
}
__device__ __forceinline__ KoImg<false> ko_image(std::false_type, const GraphView &gv, uint8_t *, uint64_t *reg) {
  return ko_glob_image(gv, reg);
}

// The dead words to zero in 16-byte stores, whole pairs, then a barrier (the global tier: behind a fence, as before
// every barrier that orders its words in device memory).  On the LDS tier the barrier also ends a staging that
// precedes it.  The caller's last reads of the words lie behind a barrier.  All 256 threads.
template <bool LDS>
__device__ __forceinline__ void ko_zero_dead(const KoImg<LDS> &g) {
  uint4 *z = reinterpret_cast<uint4 *>(g.dead);
  const uint32_t pairs = (g.V + 1u) / 2u;
  for (uint32_t i = threadIdx.x; i < pairs; i += KO_BLOCK) z[i] = make_uint4(0u, 0u, 0u, 0u);
  if (!LDS) __threadfence_block();
  __syncthreads();
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

// The lost word of a swept chunk of n hypotheses: bit b = every root (level 0) is dead under hypothesis b, the AND
// of the roots' words over the wave and then the workgroup through the four words s_w, with one barrier; the bits
// past a short chunk's n are cleared.  Behind ko_sweep's last barrier (the level offsets are staged: read behind
// a barrier).  All 256 threads, under a workgroup-uniform condition: it holds a barrier.  Every thread returns the
// word; s_w may be written again behind the caller's next barrier.
template <bool LDS>
__device__ __forceinline__ uint64_t ko_lost_word(const KoImg<LDS> &g, uint32_t n, uint64_t *s_w) {
  const uint32_t tid = threadIdx.x;
  const uint32_t n_roots = g.L ? (uint32_t)g.lvl[1] : 0u;
  uint64_t w = ~0ull;
  for (uint32_t i = tid; i < n_roots; i += KO_BLOCK) w &= g.dead[g.topo[i]];
#pragma unroll
  for (int dd = 32; dd >= 1; dd >>= 1) w &= (uint64_t)__shfl_xor((unsigned long long)w, dd);
  if (lane_id() == 0u) s_w[tid >> 6] = w;
  __syncthreads();
  const uint64_t lost = n_roots ? (s_w[0] & s_w[1] & s_w[2] & s_w[3]) : 0ull;
  return lost & (n == KO_CHUNK ? ~0ull : (1ull << n) - 1ull);
}

// lane b's return value: how many of the wave's 64 words (lo, hi) have bit b set.  Every lane takes its bit of each
// lane's word in turn; no early-out (k_knock.hip's ko_colcount is the ballot form with one).
__device__ __forceinline__ uint32_t ko_colsum(uint32_t lo, uint32_t hi) {
  const uint32_t lane = lane_id(), sh = lane & 31u;
  const bool up = lane >= 32u;
  uint32_t r = 0;
#pragma unroll
  for (int j = 0; j < 64; j++) {
    const uint32_t l0 = __builtin_amdgcn_readlane(lo, j), l1 = __builtin_amdgcn_readlane(hi, j);
    r += ((up ? l1 : l0) >> sh) & 1u;
  }
  return r;
}

// ---- host side of the launches -----------------------------------------------------------------------
// Workgroups of the persistent LDS-tier kernel f resident on n_cu CUs at lds_bytes of dynamic LDS; 0 if none.
// (The query raises the kernel's MaxDynamicSharedMemorySize, a permission, not an allocation.)
static inline uint32_t ko_lds_resident(const void *f, uint32_t lds_bytes, uint32_t n_cu) {
  int per_cu = 0;
  if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f, KO_BLOCK, lds_bytes) != hipSuccess || per_cu < 1) {
    (void)hipGetLastError();
    return 0u;
  }
  return (uint32_t)per_cu * n_cu;
}

// f(std::integral_constant<uint32_t, SIZE>) for a round's size 1, 2 or 3: one instantiation per round
template <class F>
static inline void ko_by_size(uint32_t size, F &&f) {
  if (size == 1u) f(std::integral_constant<uint32_t, 1u>{});
  else if (size == 2u) f(std::integral_constant<uint32_t, 2u>{});
  else f(std::integral_constant<uint32_t, 3u>{});
}

}  // namespace nemo
