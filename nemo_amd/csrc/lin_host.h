// lin_host.h — the arithmetic of nemo_lineage_cuts (k_lineage.hip; DESIGN.md §Lineage-driven cut search) as pure
// functions: a set of at most eight candidate positions as a key of two u64 (pack, unpack, insert, the subset a mask
// picks, the hash; the kernels call the very same code), the order of the rows (size, then colex over the candidate
// positions), the enumeration of a set's proper non-empty subsets, the validation of the candidate list (cut_host.h's,
// with the limit a u16 position sets), the limits, the sizes of the two open-addressing tables and of the emission
// buffer, and the chunk and grid counts.  No HIP and no context, so tools/lin_host_check.cpp drives it under the host
// sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "cut_host.h"    // check_cands, chunks, grid
#include "knock_host.h"  // KO_HD, KO_CHUNK

namespace lin {

#define LIN_MAX_SIZE 8u                     // a set is eight u16 positions
#define LIN_PAD 0xFFFFu                     // an unused position of a key
#define LIN_MAX_CAND 65535ull               // positions 0 .. 65534: LIN_PAD is no position
#define LIN_MAX_FRONT 0xFFFFFFFEull         // sets of one level: an index is a u32, UINT32_MAX stays free
#define LIN_CHILDREN_DEFAULT (1ull << 24)   // option lineage_children_max: 16 bytes per child, 256 MiB
#define LIN_CHILDREN_MIN 64ull
#define LIN_CHILDREN_MAX (1ull << 31)       // a table entry is a child's index + 1 in a u32
#define LIN_EMIT_START 1024ull              // children the emission buffer holds before it has grown
#define LIN_MIN_TABLE 64ull
#define LIN_BLOCK 256u                        // threads of a workgroup of k_lin_filter (KO_BLOCK)

// ---- keys ------------------------------------------------------------------------------------------------
// The set itself: its positions ascending in u16 fields 0 .. 7 (field j: bits 16 j of lo, j < 4, else of hi), the
// unused fields LIN_PAD.  Equal keys are equal sets.
struct Key {
  uint64_t lo, hi;
};
KO_HD static inline Key key_empty() { return Key{~0ull, ~0ull}; }
KO_HD static inline bool key_eq(const Key &a, const Key &b) { return a.lo == b.lo && a.hi == b.hi; }
KO_HD static inline uint32_t key_at(const Key &k, uint32_t j) {
  return (uint32_t)((j < 4u ? k.lo >> (16u * j) : k.hi >> (16u * (j - 4u))) & 0xFFFFull);
}
KO_HD static inline void key_set(Key *k, uint32_t j, uint32_t pos) {
  if (j < 4u) k->lo = (k->lo & ~(0xFFFFull << (16u * j))) | ((uint64_t)pos << (16u * j));
  else k->hi = (k->hi & ~(0xFFFFull << (16u * (j - 4u)))) | ((uint64_t)pos << (16u * (j - 4u)));
}
KO_HD static inline uint32_t key_size(const Key &k) {
  uint32_t n = 0;
  while (n < LIN_MAX_SIZE && key_at(k, n) != LIN_PAD) n++;
  return n;
}
// pos[0 .. n) ascending, n <= 8
KO_HD static inline Key key_pack(const uint32_t *pos, uint32_t n) {
  Key k = key_empty();
  for (uint32_t j = 0; j < n; j++) key_set(&k, j, pos[j]);
  return k;
}
// the positions into pos[8]; returns the size
KO_HD static inline uint32_t key_unpack(const Key &k, uint32_t *pos) {
  const uint32_t n = key_size(k);
  for (uint32_t j = 0; j < n; j++) pos[j] = key_at(k, j);
  return n;
}
// k with position p, which it does not hold, at its place; k holds fewer than eight
KO_HD static inline Key key_insert(const Key &k, uint32_t p) {
  Key out = key_empty();
  uint32_t j = 0, o = 0;
  for (; j < LIN_MAX_SIZE - 1u; j++) {
    const uint32_t x = key_at(k, j);
    if (x == LIN_PAD || x > p) break;
    key_set(&out, o++, x);
  }
  key_set(&out, o++, p);
  for (; j < LIN_MAX_SIZE - 1u; j++) {
    const uint32_t x = key_at(k, j);
    if (x == LIN_PAD) break;
    key_set(&out, o++, x);
  }
  return out;
}
// the subset of k that the bits of mask pick (bit j: field j)
KO_HD static inline Key key_subset(const Key &k, uint32_t mask) {
  Key out = key_empty();
  uint32_t o = 0;
  for (uint32_t j = 0; j < LIN_MAX_SIZE; j++)
    if ((mask >> j) & 1u) key_set(&out, o++, key_at(k, j));
  return out;
}
// The proper non-empty subsets of a set of n positions are the masks 1 .. 2^n - 2: at most 254.
KO_HD static inline uint32_t subset_masks(uint32_t n) { return n ? (1u << n) - 2u : 0u; }

KO_HD static inline uint64_t key_hash(const Key &k) {
  uint64_t x = k.lo * 0x9E3779B97F4A7C15ull ^ (k.hi + 0xD6E8FEB86659FD93ull);
  x ^= x >> 32;
  x *= 0xD6E8FEB86659FD93ull;
  x ^= x >> 29;
  x *= 0x9E3779B97F4A7C15ull;
  return x ^ (x >> 32);
}
// slots is a power of two
KO_HD static inline uint64_t first_slot(const Key &k, uint64_t slots) { return key_hash(k) & (slots - 1ull); }
KO_HD static inline uint64_t next_slot(uint64_t h, uint64_t slots) { return (h + 1ull) & (slots - 1ull); }

// ---- the rows' order -------------------------------------------------------------------------------------
// (size, colex over the candidate positions): of two sets of one size the one whose largest position is smaller
// comes first, then the next largest, and so on.  For size <= 3 this is nemo_min_cuts' (size, rank) order.
static inline bool row_less(const Key &a, const Key &b) {
  const uint32_t na = key_size(a), nb = key_size(b);
  if (na != nb) return na < nb;
  for (uint32_t j = na; j-- > 0;) {
    const uint32_t x = key_at(a, j), y = key_at(b, j);
    if (x != y) return x < y;
  }
  return false;
}

// ---- the call's checks -------------------------------------------------------------------------------------
enum CandCheck { CAND_OK = 0, CAND_RANGE = 1, CAND_DUP = 2, CAND_LIMIT = 3 };
// cut_host.h's check of the list, then the limit of a u16 position
static inline CandCheck check_cands(const uint32_t *cand, size_t n, uint64_t V, size_t *where) {
  switch (cuts::check_cands(cand, n, V, where)) {
    case cuts::CAND_RANGE:
      return CAND_RANGE;
    case cuts::CAND_DUP:
      return CAND_DUP;
    default:
      return n > LIN_MAX_CAND ? CAND_LIMIT : CAND_OK;
  }
}
static inline bool size_ok(uint32_t max_size, uint32_t flags) { return max_size >= 1 && max_size <= LIN_MAX_SIZE && flags == 0; }
static inline bool front_fits(uint64_t n) { return n <= LIN_MAX_FRONT; }

// the value nemo_set_option keeps for "lineage_children_max": -1 = the default; 0 = not a value (below 64)
static inline uint64_t children_option(int64_t value) {
  if (value == -1) return LIN_CHILDREN_DEFAULT;
  if (value < (int64_t)LIN_CHILDREN_MIN) return 0;
  return std::min<uint64_t>((uint64_t)value, LIN_CHILDREN_MAX);
}

// ---- sizes -------------------------------------------------------------------------------------------------
// An open-addressing table of u32 (index + 1, 0 = empty) for `entries` keys: a power of two, at most half full.
static inline uint64_t table_slots(uint64_t entries) {
  uint64_t s = LIN_MIN_TABLE;
  while (s < 2 * entries) s <<= 1;
  return s;
}
// the most children a level of n_front sets of size d over K candidates can emit (a set's children add a candidate
// it does not hold), saturating
static inline uint64_t emit_bound(uint64_t n_front, uint64_t K, uint32_t d) {
  const uint64_t per = K > d ? K - d : 0;
  if (per && n_front > ~0ull / per) return ~0ull;
  return n_front * per;
}
// the emission buffer after a level counted `counted` children past its `cap`: exactly the count
static inline uint64_t emit_grown(uint64_t cap, uint64_t counted) { return std::max(cap, counted); }
// the cuts' list and table before a level of n_front sets: every set may be a cut; grows by doubling at least
static inline uint64_t cuts_grown(uint64_t cap, uint64_t n_cuts, uint64_t n_front) {
  const uint64_t need = n_cuts + n_front;
  return need <= cap ? cap : std::max(need, 2 * cap);
}

// ---- a level's end -----------------------------------------------------------------------------------------
// What follows a pass over a level that counted `counted` children (before duplicates are removed; the group search:
// every list position's) behind an emission buffer of `cap`: the children are all there (LEVEL_DONE); the count
// passes the option (LEVEL_LIMIT: NEMO_ERR_LIMIT); the level runs again behind a buffer of emit_grown(cap, counted),
// its cuts in place (LEVEL_AGAIN); or, on the second pass, the count passed the grown buffer, which cannot be
// (LEVEL_BROKEN).
enum LevelEnd { LEVEL_DONE = 0, LEVEL_AGAIN = 1, LEVEL_LIMIT = 2, LEVEL_BROKEN = 3 };
static inline LevelEnd level_end(uint64_t counted, uint64_t cap, uint64_t children_max, int pass) {
  if (counted > children_max) return LEVEL_LIMIT;
  if (counted <= cap) return LEVEL_DONE;
  return pass ? LEVEL_BROKEN : LEVEL_AGAIN;
}

static inline uint64_t chunks(uint64_t n_front) { return cuts::chunks(n_front); }
// workgroups of the persistent evaluation over n chunks: cut_host.h's rule under the option kl_grid
static inline uint32_t grid(uint64_t n_chunks, uint64_t resident, uint32_t cap) { return cuts::grid(n_chunks, resident, cap); }
// workgroups of k_lin_filter over n children, `block` threads each: a grid-stride loop past `most`
static inline uint32_t filter_grid(uint64_t n, uint32_t block, uint64_t most) {
  const uint64_t g = n / block + (n % block != 0);
  return (uint32_t)std::max<uint64_t>(1, std::min(g, most ? most : 1));
}

// ---- host forms of the kernels' table steps (the check program and nothing else calls them) ---------------
// keys[i] into the table unless an equal key is there: true if it went in
static inline bool table_insert(uint32_t *tab, uint64_t slots, const Key *keys, uint32_t i) {
  uint64_t h = first_slot(keys[i], slots);
  while (tab[h]) {
    if (key_eq(keys[tab[h] - 1u], keys[i])) return false;
    h = next_slot(h, slots);
  }
  tab[h] = i + 1u;
  return true;
}
static inline bool table_has(const uint32_t *tab, uint64_t slots, const Key *keys, const Key &k) {
  uint64_t h = first_slot(k, slots);
  while (tab[h]) {
    if (key_eq(keys[tab[h] - 1u], k)) return true;
    h = next_slot(h, slots);
  }
  return false;
}
// some proper non-empty subset of k, of a size whose bit is set in sizes (bit s: cuts of size s exist), is in the table
static inline bool has_cut_subset(const uint32_t *tab, uint64_t slots, const Key *cuts_, const Key &k, uint32_t sizes) {
  const uint32_t n = key_size(k);
  for (uint32_t m = 1; m <= subset_masks(n); m++) {
    if (!((sizes >> __builtin_popcount(m)) & 1u)) continue;
    if (table_has(tab, slots, cuts_, key_subset(k, m))) return true;
  }
  return false;
}

}  // namespace lin
