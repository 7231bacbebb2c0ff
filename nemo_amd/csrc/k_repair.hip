// k_repair.hip — nemo_min_repair_sets / nemo_min_repairs (DESIGN.md §Minimal repair sets): all minimal repairs of
// size <= 3 of a raw provenance graph under an absent set A.  The monotone dual of k_cuts.hip, by the same loop in
// its repair mode (cut_dev.h).  k_repair_lds / k_repair_glob are persistent, one instantiation per round; round 0 is
// one chunk of two hypotheses, S = {} and S = every candidate.  The rows come from k_cuts.hip's k_cut_count /
// k_cut_emit.  k_repair_absent makes the pair form's absent set and candidate list.
#include "cut_dev.h"
#include "repair_host.h"

namespace nemo {

// one instantiation per round (SIZE = 0, 1, 2, 3).  The bitmap is staged once behind k_ko_lds's image
// (repair::repair_lds_bytes); the barrier behind it also ends the image's staging.
template <uint32_t SIZE>
__global__ __launch_bounds__(KO_BLOCK) void k_repair_lds(DevCorpus c, RepairArgs a) {
  extern __shared__ __align__(16) uint8_t dyn[];
  const GraphView gv = c.view(a.c.graph);
  const KoImg<true> g = ko_stage_image(gv, dyn);
  uint64_t *absent = reinterpret_cast<uint64_t *>(dyn + knock::knock_lds_bytes(gv.V, gv.E, gv.nlev));
  const uint4 *src = reinterpret_cast<const uint4 *>(a.absent);
  uint4 *dst = reinterpret_cast<uint4 *>(absent);
  const uint32_t n4 = (uint32_t)(repair::bitmap_words(gv.V) / 2u);
  for (uint32_t i = threadIdx.x; i < n4; i += KO_BLOCK) dst[i] = src[i];
  __syncthreads();
  cut_loop<true, SIZE, true>(a.c, g, absent, a.n_cand);
}

// the workgroup's own dead words in a.c.dead, the bitmap read where it lies; a fence and a barrier per level, as
// k_cut_glob.  Correct, not tuned.
template <uint32_t SIZE>
__global__ __launch_bounds__(KO_BLOCK) void k_repair_glob(DevCorpus c, RepairArgs a) {
  const GraphView gv = c.view(a.c.graph);
  const KoImg<false> g = ko_glob_image(gv, a.c.dead + (uint64_t)blockIdx.x * (((uint64_t)gv.V + 1ull) & ~1ull));
  cut_loop<false, SIZE, true>(a.c, g, a.absent, a.n_cand);
}

// ---- the pair form's absent set -----------------------------------------------------------------------
// One workgroup over the base run's post graph: a node is absent iff it is a sink goal (no rule, an empty forward
// row) whose label misses the other run's table (key = label + 1 at slot hash_label(label) & mask, 0 empty, linear
// probing: LabTab's layout).  A wave takes 64 consecutive nodes, so its ballot is one word of the bitmap; every
// word of the bitmap is written, the ones past V as 0.  A block scan per round of 256 nodes gives the absent nodes
// their positions in node-index order.  cand holds V entries.
__global__ __launch_bounds__(KO_BLOCK) void k_repair_absent(DevCorpus c, uint32_t graph, const uint32_t *key, uint32_t mask,
                                                           uint64_t *absent, uint32_t *cand, uint32_t *cnt) {
  __shared__ uint32_t s_scan[KO_BLOCK / 64];
  const GraphView gv = c.view(graph);
  const uint32_t tid = threadIdx.x, V = gv.V;
  const uint64_t nw = repair::bitmap_words(V);
  uint32_t carry = 0;
  for (uint64_t base = 0; base < 64ull * nw; base += KO_BLOCK) {
    const uint64_t v = base + tid;
    const bool in = v < V;
    const uint32_t x = in ? (uint32_t)v : V - 1u;  // V >= 1: nw is 0 otherwise
    const uint32_t w = gv.word[x], lab = gv.label[x], b = gv.fp[x], e = gv.fp[x + 1u];
    bool miss = false;
    if (in && !is_rule(w) && b == e) {
      uint32_t h = hash_label(lab) & mask;
      for (uint32_t n = 0; n <= mask; n++) {
        const uint32_t k = key[h];
        if (k == lab + 1u) break;
        if (k == 0u) {
          miss = true;
          break;
        }
        h = (h + 1u) & mask;
      }
    }
    const uint64_t m = __ballot(miss);
    if (lane_id() == 0u && (v >> 6) < nw) absent[v >> 6] = m;
    uint32_t tot;
    const uint32_t ex = block_exscan<KO_BLOCK>(miss ? 1u : 0u, &tot, s_scan) + carry;
    if (miss) cand[ex] = (uint32_t)v;
    carry += tot;
  }
  if (tid == 0) {
    cnt[0] = carry;
    cnt[1] = gv.nlev;
  }
}

// f(std::integral_constant<uint32_t, SIZE>) for a round 0, 1, 2 or 3
template <class F>
static inline void repair_by_size(uint32_t size, F &&f) {
  if (size == 0u) f(std::integral_constant<uint32_t, 0u>{});
  else ko_by_size(size, f);
}

uint32_t repair_lds_resident(uint32_t size, uint32_t lds_bytes, uint32_t n_cu) {
  const void *f = nullptr;
  repair_by_size(size, [&](auto sz) { f = (const void *)k_repair_lds<decltype(sz)::value>; });
  return ko_lds_resident(f, lds_bytes, n_cu);
}

void launch_repair_lds(const DevCorpus &c, const RepairArgs &a, uint32_t grid, uint32_t lds_bytes, hipStream_t s) {
  if (!a.c.n_chunks) return;
  repair_by_size(a.c.size, [&](auto sz) { hipLaunchKernelGGL(k_repair_lds<decltype(sz)::value>, dim3(grid), dim3(KO_BLOCK), lds_bytes, s, c, a); });
}

void launch_repair_glob(const DevCorpus &c, const RepairArgs &a, uint32_t grid, hipStream_t s) {
  if (!a.c.n_chunks) return;
  repair_by_size(a.c.size, [&](auto sz) { hipLaunchKernelGGL(k_repair_glob<decltype(sz)::value>, dim3(grid), dim3(KO_BLOCK), 0, s, c, a); });
}

void launch_repair_absent(const DevCorpus &c, uint32_t graph, const uint32_t *key, uint32_t mask, uint64_t *absent, uint32_t *cand,
                          uint32_t *cnt, hipStream_t s) {
  hipLaunchKernelGGL(k_repair_absent, dim3(1), dim3(KO_BLOCK), 0, s, c, graph, key, mask, absent, cand, cnt);
}

}  // namespace nemo
