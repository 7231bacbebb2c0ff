// wit_host.h — the arithmetic of nemo_witness_sets / nemo_witness_labels (k_witness.hip; DESIGN.md §Surviving
// derivations) as pure functions: the LDS image with the second word array and its tier, the limits of a call (rows,
// words, kept need words), where a hypothesis lies (list position, set, chunk, bit) and where its chunk's need words
// are kept, the label form's distinct labels and the rewrite of its sets as rows of them, and a workgroup's region.
// No HIP and no context, so tools/wit_host_check.cpp drives it under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "klabel_host.h"  // chunks, words_fit, table_slots, the hash
#include "knock_host.h"   // knock_lds_bytes, ko_align, dead_words, KO_MAX_HYPS, KO_MAX_DEAD_BYTES
#include "lcut_host.h"    // list_entries, region_words

namespace wit {

#define WIT_ALL 1u                 // NEMO_WIT_ALL
#define WIT_MASKS 2u               // NEMO_WIT_MASKS
#define WIT_SINKS 4u               // NEMO_WIT_SINKS
#define WIT_LDS_MAX 159744u        // largest LDS image k_wit_lds takes: a CU's 160 KiB less 4 KiB for the kernel's static LDS
#define WIT_LDS_DEFAULT WIT_LDS_MAX  // the default of option wit_lds_max: the fastest of the three measured points (DESIGN.md §Surviving derivations)
#define WIT_MAX_NEED_BYTES KO_MAX_DEAD_BYTES  // the need words a call keeps in device memory (8 V_g bytes per list position and chunk)

// k_wit_lds's image: k_ko_lds's (dead words first), then a u64 need word per node
KO_HD static inline uint32_t wit_lds_bytes(uint32_t V, uint32_t E, uint32_t L) {
  return knock::knock_lds_bytes(V, E, L) + knock::ko_align(8u * V);
}

// The LDS tier: u16 rows as k_ko_lds's, and an image of at most lds_max bytes (option wit_lds_max; 0: no graph).
static inline bool lds_fits(uint64_t V, uint64_t E, uint64_t L, uint32_t lds_max) {
  if (!lds_max || V >= 65536 || E > 65535 || L > V) return false;
  return wit_lds_bytes((uint32_t)V, (uint32_t)E, (uint32_t)L) <= lds_max;
}

// the value nemo_set_option keeps for "wit_lds_max": negative = the default, never past WIT_LDS_MAX
static inline uint32_t lds_max_option(int64_t value) {
  return value < 0 ? WIT_LDS_DEFAULT : (uint32_t)std::min<int64_t>(value, WIT_LDS_MAX);
}

// ---- limits ----------------------------------------------------------------------------------------------
// n list positions x n_sets hypotheses each: one row per hypothesis, its index a u32 with UINT32_MAX free
static inline bool rows_fit(uint64_t n, uint64_t n_sets) { return !n || !n_sets || n_sets <= KO_MAX_HYPS / n; }

// The need words a call with NEMO_WIT_MASKS keeps: dead_words(V_i) per chunk of list position i.  moff[i]: the first
// u64 of position i's words (chunk c's follow at c * dead_words(V_i)); returns false past WIT_MAX_NEED_BYTES (the
// sum saturates).  v[i]: the nodes of list position i's graph.
static inline bool need_offsets(const uint64_t *v, size_t n, uint64_t n_chunks, std::vector<uint64_t> *moff, uint64_t *total) {
  const uint64_t cap = WIT_MAX_NEED_BYTES / 8;
  uint64_t at = 0;
  bool ok = true;
  if (moff) moff->assign(n, 0);
  for (size_t i = 0; i < n; i++) {
    if (moff) (*moff)[i] = at;
    const uint64_t w = knock::dead_words(v[i]);
    if (w && n_chunks > (cap - std::min(at, cap)) / w) ok = false, at = cap;
    else at += n_chunks * w;
  }
  if (at > cap) ok = false;
  if (total) *total = ok ? at : cap + 1;
  return ok;
}

// ---- hypotheses -------------------------------------------------------------------------------------------
// Hypothesis h of a call over n_sets sets is (list position h / n_sets, set h % n_sets); the set is bit s % 64 of
// chunk s / 64.  The node-set form has one list position.
struct Hyp {
  uint64_t pos, set, chunk;
  uint32_t bit;
};
KO_HD static inline uint64_t hyp_index(uint64_t pos, uint64_t set, uint64_t n_sets) { return pos * n_sets + set; }
static inline Hyp hyp_at(uint64_t h, uint64_t n_sets) {
  Hyp x;
  x.pos = h / n_sets, x.set = h % n_sets;
  x.chunk = x.set / KO_CHUNK, x.bit = (uint32_t)(x.set % KO_CHUNK);
  return x;
}
// the first u64 of hypothesis x's chunk among the kept need words (moff: need_offsets'; V: its graph's nodes)
static inline uint64_t need_word0(const Hyp &x, const uint64_t *moff, uint64_t V) { return moff[x.pos] + x.chunk * knock::dead_words(V); }

// ---- the label form's rows -------------------------------------------------------------------------------
// The distinct labels the sets name, ascending: row r of a graph's hit list holds the nodes that carry dist[r].
static inline std::vector<uint32_t> distinct_labels(const uint32_t *labels, uint64_t n) {
  std::vector<uint32_t> d(labels, labels + n);
  std::sort(d.begin(), d.end());
  d.erase(std::unique(d.begin(), d.end()), d.end());
  return d;
}
// ... and the sets' entries rewritten as rows (every label is in dist)
static inline std::vector<uint32_t> rows_of(const uint32_t *labels, uint64_t n, const std::vector<uint32_t> &dist) {
  std::vector<uint32_t> r(n);
  for (uint64_t k = 0; k < n; k++) r[k] = (uint32_t)(std::lower_bound(dist.begin(), dist.end(), labels[k]) - dist.begin());
  return r;
}
// the host form of k_wit_table and of the kernels' probe: key = label + 1, val = row (klabel_host.h's hash)
static inline void table_fill(uint32_t *key, uint32_t *val, uint64_t slots, const std::vector<uint32_t> &dist) {
  for (size_t r = 0; r < dist.size(); r++) {
    uint64_t h = klabel::first_slot(dist[r], slots);
    while (key[h]) h = klabel::next_slot(h, slots);
    key[h] = dist[r] + 1u, val[h] = (uint32_t)r;
  }
}
static inline uint32_t table_row(const uint32_t *key, const uint32_t *val, uint64_t slots, uint32_t label) {
  uint64_t h = klabel::first_slot(label, slots);
  while (key[h] && key[h] != label + 1u) h = klabel::next_slot(h, slots);
  return key[h] ? val[h] : 0xFFFFFFFFu;
}

// ---- a workgroup's region in device memory, in u64 ---------------------------------------------------------
// The global tier keeps the dead and the need words of its graph there (words = 2 dead_words(V)); behind them, on
// either tier, the entries of the hit list that the `head` entries of LDS behind the image do not hold (the label
// form: k1 distinct labels; k1 == 0, the node-set form, keeps no list).
static inline uint64_t glob_words(uint64_t V) { return 2 * knock::dead_words(V); }
static inline uint64_t region_words(uint64_t words, uint64_t k1, uint64_t V, uint64_t head) {
  return lcuts::region_words(words, k1 ? lcuts::list_entries(k1, V) : 0, head);
}

// the byte model of one staged graph (k_ko_lds's: DESIGN.md §Knock-out) and of one chunk on it
static inline double image_bytes(double V, double E, double L) { return 4.0 * E + 12.0 * V + 4.0 * L + 8.0; }

}  // namespace wit
