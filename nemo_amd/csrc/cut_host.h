// cut_host.h — the arithmetic of nemo_min_cuts (k_cuts.hip; DESIGN.md §Minimal cut sets) as pure functions: the
// colex rank of a pair / triple of live positions and its inverse (the kernels call the very same code), the
// round-3 test for a cut pair inside a triple (k_cuts.hip and k_lcuts.hip call the very same code), the per-round
// limit, the validation of the candidate list, the live list from round 1's words, the chunk and grid counts, and
// the sizes cut_api.h's node_search takes (the global tier's resident bound, the bound of a round's hypotheses, round
// 1's words and pinned elements).  No HIP and no context, so tools/cut_host_check.cpp drives it under the host sanitizers.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "knock_host.h"  // KO_HD, KO_CHUNK

namespace cuts {

#define CUT_MAX_SIZE 3u
#define CUT_MAX_HYPS 0xFFFFFFFEull  // hypotheses of one round: a rank is a u32, UINT32_MAX stays free
#define CUT_SAT (~0ull)             // a count past u64
#define CUT_DEAD_BYTES (1ull << 30) // the dead words k_cut_glob's workgroups keep in device memory, all together

KO_HD static inline uint64_t choose2(uint64_t n) { return n < 2 ? 0 : (n & 1 ? n * ((n - 1) / 2) : (n / 2) * (n - 1)); }
// exact up to n = 2642245 (C(n,3) < 2^63 there, and the product before the last division below 2^64); CUT_SAT past it
KO_HD static inline uint64_t choose3(uint64_t n) {
  if (n < 3) return 0;
  if (n > 2642245ull) return CUT_SAT;
  return choose2(n) * (n - 2) / 3;  // C(n,2) (n - 2) = 3 C(n,3)
}

// Live positions a < b (< c) -> the hypothesis index of their set, colex: all sets below position c come first.
KO_HD static inline uint64_t rank2(uint32_t a, uint32_t b) { return choose2(b) + a; }
KO_HD static inline uint64_t rank3(uint32_t a, uint32_t b, uint32_t c) { return choose3(c) + choose2(b) + a; }

// The inverses, for h <= CUT_MAX_HYPS.  The largest b with C(b,2) <= h, the largest c with C(c,3) <= h: a float
// estimate, then integer steps to the exact value (the estimate is off by a few units at most, either way).
KO_HD static inline void unrank2(uint64_t h, uint32_t *a, uint32_t *b) {
  uint64_t y = (uint64_t)((1.0f + sqrtf(8.0f * (float)h + 1.0f)) * 0.5f);
  if (y < 1) y = 1;
  while (choose2(y) > h) y--;
  while (choose2(y + 1) <= h) y++;
  *b = (uint32_t)y;
  *a = (uint32_t)(h - choose2(y));
}
KO_HD static inline void unrank3(uint64_t h, uint32_t *a, uint32_t *b, uint32_t *c) {
  uint64_t z = (uint64_t)cbrtf(6.0f * (float)h) + 1;
  if (z < 2) z = 2;
  while (choose3(z) > h) z--;
  while (choose3(z + 1) <= h) z++;
  *c = (uint32_t)z;
  unrank2(h - choose3(z), a, b);
}

// the live positions of hypothesis h of round SIZE, by value (a < b < c; the unused ones 0)
struct Pos {
  uint32_t a, b, c;
};
template <uint32_t SIZE>
KO_HD static inline Pos unrank(uint64_t h) {
  Pos p = {(uint32_t)h, 0u, 0u};
  if (SIZE == 2u) unrank2(h, &p.a, &p.b);
  if (SIZE == 3u) unrank3(h, &p.a, &p.b, &p.c);
  return p;
}

// Round 3's test "a pair of this triple is already a cut": pairs are round 2's words, bit rank2(x, y) of them =
// "live positions x < y are a cut"; such a triple is no minimal cut.
KO_HD static inline bool has_cut_pair(const uint64_t *pairs, const Pos &p) {
  const uint64_t r0 = rank2(p.a, p.b), r1 = rank2(p.a, p.c), r2 = rank2(p.b, p.c);
  const uint64_t w0 = pairs[r0 >> 6], w1 = pairs[r1 >> 6], w2 = pairs[r2 >> 6];
  return (((w0 >> (r0 & 63u)) | (w1 >> (r1 & 63u)) | (w2 >> (r2 & 63u))) & 1ull) != 0ull;
}

// hypotheses of round `size` (1..3) over k live candidates; CUT_SAT where the count does not fit
static inline uint64_t round_hyps(uint64_t k, uint32_t size) {
  if (size == 1) return k;
  if (size == 2) return k > 0xFFFFFFFFull ? CUT_SAT : choose2(k);
  return choose3(k);
}
static inline bool round_fits(uint64_t k, uint32_t size) { return round_hyps(k, size) <= CUT_MAX_HYPS; }

enum CandCheck { CAND_OK = 0, CAND_RANGE = 1, CAND_DUP = 2 };

// The candidate list: every node < V, no node twice.  *where is the position of the first offence (for a
// duplicate: of its second occurrence).
static inline CandCheck check_cands(const uint32_t *cand, size_t n, uint64_t V, size_t *where) {
  for (size_t i = 0; i < n; i++)
    if (cand[i] >= V) {
      if (where) *where = i;
      return CAND_RANGE;
    }
  if (n > V) {  // more candidates than nodes: some node twice, within the first V + 1
    n = (size_t)V + 1;
  }
  std::vector<uint64_t> key(n);  // node << 32 | position (a position fits: n <= V + 1 <= 2^32)
  for (size_t i = 0; i < n; i++) key[i] = ((uint64_t)cand[i] << 32) | (uint64_t)(uint32_t)i;
  std::sort(key.begin(), key.end());
  size_t first = n;
  for (size_t i = 1; i < n; i++)
    if ((key[i] >> 32) == (key[i - 1] >> 32)) first = std::min(first, (size_t)(uint32_t)key[i]);
  if (first < n) {
    if (where) *where = first;
    return CAND_DUP;
  }
  return CAND_OK;
}

static inline uint64_t chunks(uint64_t n_hyp) { return n_hyp / KO_CHUNK + (n_hyp % KO_CHUNK != 0); }

// The live list: the candidate positions whose singleton is no cut, in candidate order.  words: round 1's
// result, bit p of word p / 64 = "candidate p alone is a cut".
static inline std::vector<uint32_t> live_list(const uint64_t *words, size_t k) {
  std::vector<uint32_t> live;
  for (size_t p = 0; p < k; p++)
    if (!((words[p / 64] >> (p % 64)) & 1ull)) live.push_back((uint32_t)p);
  return live;
}

// Workgroups of a persistent launch over n chunks: as many as are resident on the device, capped by the option
// cut_grid (0: no cap); at least one.
static inline uint32_t grid(uint64_t n_chunks, uint64_t resident, uint32_t cap) {
  uint64_t g = std::min(n_chunks, resident ? resident : 1);
  if (cap) g = std::min<uint64_t>(g, cap);
  return (uint32_t)std::max<uint64_t>(g, 1);
}

// ---- the sizes of a search over one graph (cut_api.h's node_search) ---------------------------------------
// The global tier's resident workgroups, untuned: two per CU, fewer where their dead words (dead_words u64 each)
// would pass CUT_DEAD_BYTES all together; at least one.
static inline uint64_t glob_resident(uint32_t n_cu, uint64_t dead_words) {
  return std::max<uint64_t>(1, std::min<uint64_t>(2ull * n_cu, CUT_DEAD_BYTES / (8 * std::max<uint64_t>(dead_words, 1))));
}

// An upper bound of any round's hypotheses over K candidates, before the live list is known; at least one.
static inline uint64_t most_hyps(uint64_t K, uint32_t max_size) {
  uint64_t most = std::max<uint64_t>(K, 1);
  for (uint32_t sz = 2; sz <= max_size; sz++) most = std::max(most, std::min<uint64_t>(round_hyps(K, sz), CUT_MAX_HYPS));
  return most;
}

// Round 1's words, with round 0's one word behind them where the search has a round 0; and the u32 elements of the
// pinned buffer that takes those words, the K candidates behind them and the call's 8 counts.
static inline uint64_t first_words(uint64_t K, bool round0) { return chunks(K) + (round0 ? 1 : 0); }
static inline uint64_t first_pinned(uint64_t K, bool round0) { return 2 * first_words(K, round0) + K + 8; }

}  // namespace cuts
