// lgc_host.h — the arithmetic of nemo_lineage_group_cuts (k_lgcuts.hip; DESIGN.md §Lineage cut search over fault
// events) as pure functions: the limits of the call and of a level, what a workgroup keeps behind its LDS image (the
// rows' need words, then the head of the hit list) and in its region of device memory, the cross-run count that makes
// a set a cut, and the most children a level can count.  The keys, the tables, the rows' order, the emission buffer
// and the rule by which a level runs again are lin_host.h's, the groups' checks gcut_host.h's, the work items klabel_host.h's, the image wit_host.h's.
// No HIP and no context, so tools/lgc_host_check.cpp drives it under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gcut_host.h"
#include "lin_host.h"
#include "wit_host.h"

namespace lgc {

#define LGC_MAX_GROUPS LIN_MAX_CAND  // a set is eight u16 candidate positions

static inline bool groups_fit(uint64_t n_groups) { return n_groups <= LGC_MAX_GROUPS; }
static inline bool size_ok(uint32_t max_size) { return max_size >= 1 && max_size <= LIN_MAX_SIZE; }

// A level of n_front sets on n list positions: one lost word per (list position, chunk of 64 sets), at most
// KL_MAX_WORDS of them; and a frontier index is a u32 (lin::front_fits).
enum LevelCheck { LEVEL_OK = 0, LEVEL_FRONT = 1, LEVEL_WORDS = 2 };
static inline LevelCheck level_check(uint64_t n, uint64_t n_front) {
  if (!lin::front_fits(n_front)) return LEVEL_FRONT;
  if (!klabel::words_fit(n, n_front)) return LEVEL_WORDS;
  return LEVEL_OK;
}

// ---- what a workgroup keeps behind the image ---------------------------------------------------------------
// Of the launch's dynamic LDS the graph's image (wit_host.h: graph, dead words, need words) takes `image` bytes.  What
// is left holds the need words of the D rows (a u64 per distinct label), if all of them fit, and then the head of the
// hit list (u32 entries).  The kernels and the host call the very same function.
struct Tail {
  uint32_t rn_lds;    // 1: the rows' need words are in LDS, at `image`
  uint32_t rn_bytes;  // ... and take this much of it (whole 16-byte chunks)
  uint32_t head;      // hit-list entries in LDS behind them
};
KO_HD static inline Tail tail(uint32_t lds_total, uint32_t image, uint32_t D) {
  Tail t;
  const uint32_t left = lds_total > image ? lds_total - image : 0u;
  const uint64_t rn = ((uint64_t)8u * D + 15u) & ~15ull;
  t.rn_lds = rn <= left ? 1u : 0u;
  t.rn_bytes = t.rn_lds ? (uint32_t)rn : 0u;
  t.head = (left - t.rn_bytes) / 4u;
  return t;
}
// the bytes a launch asks for behind its largest image: the rows' need words and the whole hit list
static inline uint64_t tail_want(uint64_t D, uint64_t V) { return ((8 * D + 15) & ~15ull) + 4 * gcuts::list_entries(D, V); }

// A workgroup's region in device memory, in u64: the global tier's dead and need words (words = wit::glob_words(V),
// 0 on the LDS tier), the rows' need words unless LDS holds them, and the hit-list entries past the head.
KO_HD static inline uint64_t rn_words(uint64_t D) { return (D + 1) & ~1ull; }
KO_HD static inline uint64_t rn_offset(uint64_t words) { return (words + 1) & ~1ull; }
KO_HD static inline uint64_t spill_offset(uint64_t words, uint64_t D, const Tail &t) { return rn_offset(words) + (t.rn_lds ? 0 : rn_words(D)); }
static inline uint64_t region_words(uint64_t words, uint64_t D, uint64_t V, const Tail &t) {
  const uint64_t entries = gcuts::list_entries(D, V);
  const uint64_t spill = entries > t.head ? entries - t.head : 0;
  return spill_offset(words, D, t) + (((spill + 1) / 2 + 1) & ~1ull);
}

// ---- the cross-run count -----------------------------------------------------------------------------------
// lost: [n][n_chunks] the level's lost words; set s is bit s % 64 of chunk s / 64.  A run listed twice has two list
// positions and counts twice.
KO_HD static inline uint32_t lost_count(const uint64_t *lost, uint64_t n, uint64_t n_chunks, uint64_t s) {
  uint32_t cnt = 0;
  for (uint64_t i = 0; i < n; i++) cnt += (uint32_t)((lost[i * n_chunks + s / KO_CHUNK] >> (s % KO_CHUNK)) & 1ull);
  return cnt;
}
KO_HD static inline bool is_cut(uint32_t count, uint32_t q) { return q > 0 && count >= q; }

// ---- a level's children ------------------------------------------------------------------------------------
// the most children a level can count: every list position emits every (set, candidate outside it) at most once
static inline uint64_t emit_bound(uint64_t n, uint64_t n_front, uint64_t K, uint32_t d) {
  const uint64_t one = lin::emit_bound(n_front, K, d);
  if (n && one > ~0ull / n) return ~0ull;
  return one * n;
}

}  // namespace lgc
