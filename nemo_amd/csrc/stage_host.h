// stage_host.h — host arithmetic of the sliced hand-over (nemo_stage_simplified, option stage_slices):
// which part of the node state's words, or of the chain pairs, each slice packs and copies.  Pure host
// code, no HIP: tools/stage_host_check.cpp drives it under the host sanitizers.
#pragma once
#include <cstdint>

#define NEMO_STAGE_SLICES_MAX 8u
#define NEMO_STAGE_SLICES_DEFAULT 2u  // the step time at 1, 2, 3, 4 and 8 slices
#define NEMO_STAGE_RATIO_MAX 8u
#define NEMO_STAGE_RATIO_DEFAULT 4u       // each slice of the node state four times the one before
#define NEMO_STAGE_PAIR_SLICES_DEFAULT 1u  // the pairs are ready before the state's copies end: one copy

namespace stage {

// Slice k of K over [0, n), the slices' lengths growing by the factor `ratio` from one to the next
// (ratio 1: nearly equal, [floor(k n / K), floor((k + 1) n / K)), lengths within one of each other).
// The K ranges tile [0, n) in order, each element exactly once; with K > n some are empty.
// A first slice shorter than the rest puts the link to work sooner: its kernel is the only one no
// copy runs beside.  A slice's kernel must still end before the copy of the slice before it does, so
// the ratio stays under copy time over kernel time.
static inline uint64_t slice_lo(uint64_t n, uint32_t K, uint32_t k, uint32_t ratio = 1) {
  unsigned __int128 sk = 0, sK = 0, w = 1;  // sums of ratio^i over i < k and over i < K (ratio, K <= 8: under 2^25)
  for (uint32_t i = 0; i < K; i++, w *= ratio) {
    if (i < k) sk += w;
    sK += w;
  }
  return k >= K ? n : (uint64_t)((unsigned __int128)n * sk / sK);
}

struct Range {
  uint64_t lo, hi;
  bool empty() const { return lo >= hi; }
  uint64_t size() const { return hi - lo; }
};

static inline Range slice(uint64_t n, uint32_t K, uint32_t k, uint32_t ratio = 1) {
  return {slice_lo(n, K, k, ratio), slice_lo(n, K, k + 1, ratio)};
}

// the option's value as a slice count: 1..NEMO_STAGE_SLICES_MAX
static inline uint32_t clamp_slices(int64_t v, uint32_t dflt) {
  if (v < 0) return dflt;
  if (v < 1) return 1u;
  return v > (int64_t)NEMO_STAGE_SLICES_MAX ? NEMO_STAGE_SLICES_MAX : (uint32_t)v;
}

// u32 words of the 2-bit node state of V nodes (16 nodes per word; the tail word is the last slice's)
static inline uint64_t state_words(uint64_t V) { return V / 16 + (V % 16 != 0); }

// nodes whose flags the words [w.lo, w.hi) of the state of V nodes pack
static inline uint64_t state_nodes(uint64_t V, Range w) {
  const uint64_t a = 16 * w.lo < V ? 16 * w.lo : V, b = w.hi >= state_words(V) ? V : 16 * w.hi;
  return b > a ? b - a : 0;
}

}  // namespace stage
