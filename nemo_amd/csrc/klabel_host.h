// klabel_host.h — the arithmetic of nemo_knockout_labels (k_klabel.hip; DESIGN.md §Knock-out by label) as pure
// functions: the validation of the label sets and the two limits of a call, the sizes and offsets of the
// per-chunk label tables (from set_off alone), the hash the host and the kernels share, the cut of the call into
// work items (list position, chunk range) and the grid.  No HIP and no context, so tools/klabel_host_check.cpp
// drives it under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "knock_host.h"  // KO_HD, KO_CHUNK

namespace klabel {

#define KL_SINKS 1u                      // NEMO_KL_SINKS
#define KL_MAX_WORDS (1ull << 28)        // n * n_chunks: (lost, hit) word pairs of one call
#define KL_MAX_LABELS 0xFFFFFFFFull      // labels named by the sets of one call
#define KL_MAX_SETS 0xFFFFFFFFull        // sets of one call
#define KL_NO_LABEL 0xFFFFFFFFu          // no legal label: label + 1 is the table key, 0 the empty slot
#define KL_MIN_TABLE 16ull               // slots of the smallest table (a power of two)
#define KL_REGION_BYTES (1ull << 30)     // the workgroups' regions of a launch in device memory, all together

static inline uint64_t chunks(uint64_t n_sets) { return n_sets / KO_CHUNK + (n_sets % KO_CHUNK != 0); }

enum SetCheck { SET_OK = 0, SET_NONMONOTONE = 1, SET_LABEL = 2, SET_LIMIT = 3 };

// The offsets alone: set_off must not decrease and the sets may name at most KL_MAX_LABELS labels in all.
// Reads set_off[0 .. n_sets] and nothing else.  *where: the first decreasing set.
static inline SetCheck check_offsets(const uint64_t *set_off, size_t n_sets, uint64_t *where) {
  for (size_t s = 0; s < n_sets; s++)
    if (set_off[s + 1] < set_off[s]) {
      if (where) *where = s;
      return SET_NONMONOTONE;
    }
  if (n_sets && set_off[n_sets] - set_off[0] > KL_MAX_LABELS) return SET_LIMIT;
  return SET_OK;
}

// The sets of nemo_knockout_labels: set s is set_labels[set_off[s] .. set_off[s + 1]).  The offsets are checked
// first (so a call past the label limit reads no label), then every label must differ from KL_NO_LABEL.
// *where: the set (SET_NONMONOTONE) or the position in set_labels (SET_LABEL) of the first offence.
static inline SetCheck check_sets(const uint64_t *set_off, const uint32_t *set_labels, size_t n_sets, uint64_t *where) {
  const SetCheck off = check_offsets(set_off, n_sets, where);
  if (off != SET_OK || !n_sets) return off;
  for (uint64_t k = set_off[0]; k < set_off[n_sets]; k++)
    if (set_labels[k] == KL_NO_LABEL) {
      if (where) *where = k;
      return SET_LABEL;
    }
  return SET_OK;
}

// the sets of one call: a set index is a u32 on the device (empty sets name no label, so the label limit does not
// bound them)
static inline bool sets_fit(uint64_t n_sets) { return n_sets <= KL_MAX_SETS; }

// n list positions times the chunks of n_sets within KL_MAX_WORDS
static inline bool words_fit(uint64_t n, uint64_t n_sets) {
  const uint64_t ck = chunks(n_sets);
  return !n || !ck || ck <= KL_MAX_WORDS / n;
}

// Slots of an open-addressed table of `entries` label entries (duplicates included): a power of two, at least
// twice the entries (load <= 1/2, so a probe chain ends), at least KL_MIN_TABLE.  entries <= KL_MAX_LABELS.
static inline uint64_t table_slots(uint64_t entries) {
  uint64_t s = KL_MIN_TABLE;
  while (s < 2 * entries) s <<= 1;
  return s;
}

// Table c of a call is chunk c's (label -> mask over its 64 sets), table n_chunks the union filter of all named
// labels; off[c] is its first slot in the key (and mask) array, off[n_chunks + 1] the slots in all.  From set_off
// alone: no label is read.
static inline std::vector<uint64_t> table_offsets(const uint64_t *set_off, size_t n_sets) {
  const uint64_t ck = chunks(n_sets);
  std::vector<uint64_t> off(ck + 2, 0);
  for (uint64_t c = 0; c < ck; c++) {
    const uint64_t lo = c * KO_CHUNK, hi = std::min<uint64_t>(lo + KO_CHUNK, n_sets);
    off[c + 1] = off[c] + table_slots(set_off[hi] - set_off[lo]);
  }
  off[ck + 1] = off[ck] + table_slots(n_sets ? set_off[n_sets] - set_off[0] : 0);
  return off;
}

// slot hash of a label (device.h hash_label), key = label + 1, 0 = empty, linear probing: as load_host.h's
// table of run 0
KO_HD static inline uint32_t hash(uint32_t x) {
  x *= 0x9E3779B1u;
  return x ^ (x >> 15);
}
KO_HD static inline uint64_t first_slot(uint32_t label, uint64_t slots) { return (uint64_t)hash(label) & (slots - 1); }
KO_HD static inline uint64_t next_slot(uint64_t slot, uint64_t slots) { return (slot + 1) & (slots - 1); }

// host forms of the kernels' insert and probe (the check program and the tests' reference of the table)
static inline void insert(uint32_t *key, uint64_t *mask, uint64_t slots, uint32_t label, uint64_t bits) {
  uint64_t h = first_slot(label, slots);
  while (key[h] && key[h] != label + 1u) h = next_slot(h, slots);
  key[h] = label + 1u;
  if (mask) mask[h] |= bits;
}
static inline bool probe(const uint32_t *key, const uint64_t *mask, uint64_t slots, uint32_t label, uint64_t *bits) {
  uint64_t h = first_slot(label, slots);
  while (key[h] && key[h] != label + 1u) h = next_slot(h, slots);
  if (!key[h]) return false;
  if (bits) *bits = mask ? mask[h] : 0;
  return true;
}

// Work items.  With `resident` workgroups and n listed graphs (of one tier), each graph's n_chunks are cut into
// parts = min(n_chunks, max(1, ceil(resident / n))) contiguous ranges; item t is (graph t / parts, range t % parts).
struct Split {
  uint64_t n = 0, n_chunks = 0;
  uint32_t parts = 0;
  uint64_t items = 0;  // n * parts
};
static inline Split split(uint64_t n, uint64_t n_chunks, uint64_t resident) {
  Split s;
  s.n = n, s.n_chunks = n_chunks;
  if (!n || !n_chunks) return s;
  if (!resident) resident = 1;
  const uint64_t per = std::max<uint64_t>(1, resident / n + (resident % n != 0));
  s.parts = (uint32_t)std::min<uint64_t>(n_chunks, std::min<uint64_t>(per, 0xFFFFFFFFull));
  s.items = n * s.parts;
  return s;
}
// range `part` of `parts` over n_chunks: [lo, hi), sizes differing by one at most, none empty (parts <= n_chunks)
KO_HD static inline uint32_t range_lo(uint32_t n_chunks, uint32_t parts, uint32_t part) {
  return (uint32_t)((uint64_t)n_chunks * part / parts);
}
// A workgroup takes a contiguous block of items, so that one that walks several ranges of a graph stages it once:
// workgroup b of `grid` takes items [item_lo(b), item_lo(b + 1)).
KO_HD static inline uint64_t item_lo(uint64_t items, uint32_t grid, uint32_t b) {
  return items / grid * b + (items % grid < b ? items % grid : b);
}

// Workgroups of a persistent launch over `items`: as many as are resident, capped by the option kl_grid (0: no
// cap); at least one.
static inline uint32_t grid(uint64_t items, uint64_t resident, uint32_t cap) {
  uint64_t g = std::min(items, resident ? resident : 1);
  if (cap) g = std::min<uint64_t>(g, cap);
  return (uint32_t)std::max<uint64_t>(std::min<uint64_t>(g, 0x7FFFFFFFull), 1);
}

// A workgroup's region in device memory: the hit list's (node, label) pairs that the LDS tail does not hold
// (`spill` pairs) and, on the global tier, the dead words of its graph (`dead` words), in u64.
static inline uint64_t region_words(uint64_t dead, uint64_t spill) { return ((dead + 1) & ~1ull) + ((spill + 1) & ~1ull); }
// ... and the workgroups whose regions stay within KL_REGION_BYTES (at least one)
static inline uint64_t region_grid(uint64_t resident, uint64_t words) {
  if (!words) return resident ? resident : 1;
  return std::max<uint64_t>(1, std::min<uint64_t>(resident ? resident : 1, KL_REGION_BYTES / (8 * words)));
}

}  // namespace klabel
