// repair_host.h — the host arithmetic of nemo_min_repair_sets / nemo_min_repairs (k_repair.hip; DESIGN.md §Minimal
// repair sets) as pure functions: the validation of the absent and the candidate list, the absent bitmap (a bit
// per node, whole 16-byte pairs of u64 words) and its size, k_repair_lds's LDS image and its tier, and the status
// round 0's word decides.  The ranks, the live list, the chunk and grid counts are cut_host.h's, unchanged.
// No HIP and no context, so tools/repair_host_check.cpp drives it under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "knock_host.h"  // KO_HD, ko_align, knock_lds_bytes

namespace repair {

#define REPAIR_HOLDS 0u     // NEMO_REPAIR_HOLDS
#define REPAIR_SEARCHED 1u  // NEMO_REPAIR_SEARCHED
#define REPAIR_BEYOND 2u    // NEMO_REPAIR_BEYOND

// u64 words of the absent bitmap of a graph of V nodes: a bit per node, whole 16-byte pairs (the kernels copy and
// read it in 16-byte loads); the bits past V are 0
KO_HD static inline uint64_t bitmap_words(uint64_t V) { return (((V + 63) / 64) + 1) & ~1ull; }

// k_repair_lds's image: k_ko_lds's (knock_host.h) and the absent bitmap behind it
KO_HD static inline uint32_t repair_lds_bytes(uint32_t V, uint32_t E, uint32_t L) {
  return knock::knock_lds_bytes(V, E, L) + 8u * (uint32_t)bitmap_words(V);
}

// The LDS tier: knock::lds_fits' rule on the larger image (option knock_lds_max; 0: no graph).
static inline bool lds_fits(uint64_t V, uint64_t E, uint64_t L, uint32_t lds_max) {
  if (!lds_max || V >= 65536 || E > 65535 || L > V) return false;
  return repair_lds_bytes((uint32_t)V, (uint32_t)E, (uint32_t)L) <= lds_max;
}

// the bitmap of the absent list (checked: every node < V)
static inline std::vector<uint64_t> bitmap(const uint32_t *absent, size_t n, uint64_t V) {
  std::vector<uint64_t> w(bitmap_words(V), 0ull);
  for (size_t i = 0; i < n; i++) w[absent[i] >> 6] |= 1ull << (absent[i] & 63u);
  return w;
}

enum ListCheck { LIST_OK = 0, ABSENT_RANGE = 1, ABSENT_DUP = 2, CAND_DUP = 3, CAND_NOT_ABSENT = 4 };

// the position of the first node of list[0 .. n) that comes a second time (of its second occurrence); n if none
static inline size_t first_dup(const uint32_t *list, size_t n) {
  std::vector<uint64_t> key(n);  // node << 32 | position
  for (size_t i = 0; i < n; i++) key[i] = ((uint64_t)list[i] << 32) | (uint64_t)(uint32_t)i;
  std::sort(key.begin(), key.end());
  size_t first = n;
  for (size_t i = 1; i < n; i++)
    if ((key[i] >> 32) == (key[i - 1] >> 32)) first = std::min(first, (size_t)(uint32_t)key[i]);
  return first;
}

// The two lists of nemo_min_repair_sets, in this order: every absent node < V (ABSENT_RANGE), no absent node twice
// (ABSENT_DUP), no candidate twice (CAND_DUP), every candidate an absent node (CAND_NOT_ABSENT).  cand == nullptr:
// the candidates are the absent list itself, nothing more to check.  *where is the position of the first offence
// in its own list (for a duplicate: of its second occurrence).
static inline ListCheck check_lists(const uint32_t *absent, size_t n_absent, const uint32_t *cand, size_t n_cand, uint64_t V,
                                    size_t *where) {
  for (size_t i = 0; i < n_absent; i++)
    if (absent[i] >= V) {
      if (where) *where = i;
      return ABSENT_RANGE;
    }
  // more entries than nodes: some node twice, within the first V + 1 (a position then fits 32 bits)
  size_t d = first_dup(absent, n_absent > V ? (size_t)V + 1 : n_absent);
  if (d < (n_absent > V ? (size_t)V + 1 : n_absent)) {
    if (where) *where = d;
    return ABSENT_DUP;
  }
  if (!cand) return LIST_OK;
  // a candidate list longer than the absent list names some node twice or a node that is not absent, within its
  // first n_absent + 1 entries
  const size_t n = n_cand > n_absent ? n_absent + 1 : n_cand;
  d = first_dup(cand, n);
  const std::vector<uint64_t> bits = bitmap(absent, n_absent, V);
  size_t out = n;
  for (size_t i = 0; i < n && out == n; i++)
    if (cand[i] >= V || !((bits[cand[i] >> 6] >> (cand[i] & 63u)) & 1ull)) out = i;
  if (d < n) {
    if (where) *where = d;
    return CAND_DUP;
  }
  if (out < n) {
    if (where) *where = out;
    return CAND_NOT_ABSENT;
  }
  return LIST_OK;
}

// Round 0's word: bit 0 = the outcome holds under S = {} (nothing restored), bit 1 = it holds under S = cand.
static inline uint32_t status(uint64_t word0) {
  if (word0 & 1ull) return REPAIR_HOLDS;
  return (word0 & 2ull) ? REPAIR_SEARCHED : REPAIR_BEYOND;
}

}  // namespace repair
