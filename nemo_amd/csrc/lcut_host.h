// lcut_host.h — the arithmetic of nemo_min_label_cuts (k_lcuts.hip; DESIGN.md §Minimal cut sets by label) as pure
// functions: the validation of the candidate labels, the min_runs rule, the two limits of a round, the live list
// from round 1's cut and any-hit words, and the sizes of the label -> position table and of a workgroup's region.
// The colex ranks and the round sizes are cut_host.h's, the table, the hash and the work items klabel_host.h's.
// No HIP and no context, so tools/lcut_host_check.cpp drives it under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "cut_host.h"
#include "klabel_host.h"

namespace lcuts {

#define LC_NONE 0xFFFFFFFFu  // no live position (a candidate that is not live), no label

// The candidate labels: distinct, none equal to UINT32_MAX (no label: label + 1 is the table key).  cut_host.h's
// check over the universe of all labels below UINT32_MAX.  *where: the position of the first offence.
static inline cuts::CandCheck check_cands(const uint32_t *cand, size_t n, size_t *where) {
  return cuts::check_cands(cand, n, 0xFFFFFFFFull, where);
}

// q of the call: min_runs == 0 means every list position; false: min_runs exceeds n
static inline bool min_runs(uint64_t n, uint32_t min_runs_arg, uint32_t *q) {
  if (min_runs_arg > n) return false;
  if (q) *q = min_runs_arg ? min_runs_arg : (uint32_t)n;
  return true;
}

enum RoundCheck { ROUND_OK = 0, ROUND_HYPS = 1, ROUND_WORDS = 2 };

// A round of `size` over k live candidates on n list positions: at most CUT_MAX_HYPS hypotheses, at most
// KL_MAX_WORDS lost words (one per list position and chunk of 64 hypotheses).
static inline RoundCheck round_check(uint64_t n, uint64_t k, uint32_t size) {
  if (!cuts::round_fits(k, size)) return ROUND_HYPS;
  if (!klabel::words_fit(n, cuts::round_hyps(k, size))) return ROUND_WORDS;
  return ROUND_OK;
}

// The live list: the candidate positions that are no cut alone and hit some listed graph, in candidate order.
// cut / hit: round 1's words, bit p of word p / 64.
static inline std::vector<uint32_t> live_list(const uint64_t *cut, const uint64_t *hit, size_t k) {
  std::vector<uint32_t> live;
  for (size_t p = 0; p < k; p++)
    if (!((cut[p / 64] >> (p % 64)) & 1ull) && ((hit[p / 64] >> (p % 64)) & 1ull)) live.push_back((uint32_t)p);
  return live;
}

// candidate position -> live position, LC_NONE for a candidate that is not live
static inline std::vector<uint32_t> live_map(const std::vector<uint32_t> &live, size_t k) {
  std::vector<uint32_t> map(k, LC_NONE);
  for (size_t p = 0; p < live.size(); p++) map[live[p]] = (uint32_t)p;
  return map;
}

// slots of the call's label -> candidate position table (k distinct labels)
static inline uint64_t table_slots(uint64_t k) { return klabel::table_slots(k); }

// A graph's hit list as the sweeps keep it: k1 + 1 row offsets, then at most V nodes, u32 each.  `head` of them
// stay in LDS behind the image; the u64 words a workgroup's region needs for the others, behind `dead` dead words.
static inline uint64_t list_entries(uint64_t k1, uint64_t V) { return k1 + 1 + V; }
static inline uint64_t region_words(uint64_t dead, uint64_t entries, uint64_t head) {
  const uint64_t spill = entries > head ? entries - head : 0;
  return ((dead + 1) & ~1ull) + (((spill + 1) / 2 + 1) & ~1ull);
}

}  // namespace lcuts
