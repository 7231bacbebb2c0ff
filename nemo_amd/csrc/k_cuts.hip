// k_cuts.hip — nemo_min_cuts (DESIGN.md §Minimal cut sets): all minimal cuts of size <= 3 of a raw provenance
// graph read as an AND/OR circuit.  A round's hypotheses are the sets of 1, 2 or 3 live candidates in colex rank
// order (cut_host.h), so a workgroup makes the seeds of a chunk of 64 hypotheses from the chunk's index alone.
// k_cut_lds is the persistent form of k_ko_lds: it stages the graph's LDS image once and runs cut_dev.h's loop over
// the round's chunks, the knock-out sweep on each; a chunk's result is one word, the AND of the root words.
// k_cut_glob is the same loop over the CSR in device memory.  k_cut_count / k_cut_emit turn the rounds' words
// into nemo_cut rows in (size, rank) order (the repair searches' rows too).
#include "cut_dev.h"

namespace nemo {

// one instantiation per round (SIZE = 1, 2, 3)
template <uint32_t SIZE>
__global__ __launch_bounds__(KO_BLOCK) void k_cut_lds(DevCorpus c, CutArgs a) {
  extern __shared__ __align__(16) uint8_t dyn[];
  const KoImg<true> g = ko_stage_image(c.view(a.graph), dyn);  // once; the loop's first barrier ends the staging
  cut_loop<true, SIZE, false>(a, g, nullptr, 0u);
}

// the workgroup's own dead words in a.dead; a fence and a barrier per level, as k_ko_glob.  Correct, not tuned.
template <uint32_t SIZE>
__global__ __launch_bounds__(KO_BLOCK) void k_cut_glob(DevCorpus c, CutArgs a) {
  const GraphView gv = c.view(a.graph);
  const KoImg<false> g = ko_glob_image(gv, a.dead + (uint64_t)blockIdx.x * (((uint64_t)gv.V + 1ull) & ~1ull));
  cut_loop<false, SIZE, false>(a, g, nullptr, 0u);
}

// ---- the rows -------------------------------------------------------------------------------------
__global__ __launch_bounds__(KO_BLOCK) void k_cut_count(CutArgs a) {
  const uint32_t k = blockIdx.x * KO_BLOCK + threadIdx.x;
  if (k < a.n_chunks) a.scan[k] = (uint32_t)__popcll(a.words[k]);
  if (k == a.n_chunks) a.scan[k] = 0u;
}

// A wave per word, a lane per bit: a set bit's row is the word's first row (the scan) plus the set bits below it.
__global__ __launch_bounds__(KO_BLOCK) void k_cut_emit(CutArgs a) {
  const uint32_t k = blockIdx.x * (KO_BLOCK / 64) + (threadIdx.x >> 6), lane = lane_id();
  if (k >= a.n_chunks) return;
  const uint64_t w = a.words[k];
  if (!((w >> lane) & 1ull)) return;
  const uint64_t h = (uint64_t)k * KO_CHUNK + lane;
  const cuts::Pos p = a.size == 1u ? cuts::unrank<1>(h) : a.size == 2u ? cuts::unrank<2>(h) : cuts::unrank<3>(h);
  const uint64_t r = (uint64_t)a.scan[k] + (uint32_t)__popcll(w & ((1ull << lane) - 1ull));
  uint4 row = make_uint4(a.size, NEMO_NONE, NEMO_NONE, NEMO_NONE);
  row.y = a.cand[a.live ? a.live[p.a] : p.a];  // live position -> candidate -> node (round 1: every candidate is live)
  if (a.size >= 2u) row.z = a.cand[a.live[p.b]];
  if (a.size >= 3u) row.w = a.cand[a.live[p.c]];
  reinterpret_cast<uint4 *>(a.rows)[r] = row;
}

uint32_t cut_lds_resident(uint32_t size, uint32_t lds_bytes, uint32_t n_cu) {
  const void *f = nullptr;
  ko_by_size(size, [&](auto sz) { f = (const void *)k_cut_lds<decltype(sz)::value>; });
  return ko_lds_resident(f, lds_bytes, n_cu);
}

void launch_cut_lds(const DevCorpus &c, const CutArgs &a, uint32_t grid, uint32_t lds_bytes, hipStream_t s) {
  if (!a.n_chunks) return;
  ko_by_size(a.size, [&](auto sz) { hipLaunchKernelGGL(k_cut_lds<decltype(sz)::value>, dim3(grid), dim3(KO_BLOCK), lds_bytes, s, c, a); });
}

void launch_cut_glob(const DevCorpus &c, const CutArgs &a, uint32_t grid, hipStream_t s) {
  if (!a.n_chunks) return;
  ko_by_size(a.size, [&](auto sz) { hipLaunchKernelGGL(k_cut_glob<decltype(sz)::value>, dim3(grid), dim3(KO_BLOCK), 0, s, c, a); });
}

void launch_cut_count(const CutArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_cut_count, dim3(a.n_chunks / KO_BLOCK + 1u), dim3(KO_BLOCK), 0, s, a);
}

void launch_cut_emit(const CutArgs &a, hipStream_t s) {
  if (!a.n_chunks) return;
  hipLaunchKernelGGL(k_cut_emit, dim3((a.n_chunks + KO_BLOCK / 64 - 1u) / (KO_BLOCK / 64)), dim3(KO_BLOCK), 0, s, a);
}

}  // namespace nemo
