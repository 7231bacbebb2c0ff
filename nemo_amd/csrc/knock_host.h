// knock_host.h — the host side of nemo_knockout_leaves / nemo_knockout_sets (k_knock.hip; DESIGN.md
// §Knock-out) as pure functions: the size of k_ko_lds's LDS image and its tier, the two limits of a call,
// the chunk table (one row per 64 hypotheses of one graph), and the validation of the explicit sets.
// No HIP and no context, so tools/knock_host_check.cpp drives it under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#ifdef __HIPCC__
#define KO_HD __host__ __device__
#else
#define KO_HD
#endif

namespace knock {

#define KO_CHUNK 64u                      // hypotheses per chunk: one bit column each of a u64 word per node
#define KO_MAX_HYPS 0xFFFFFFFEull         // hypotheses of one call (UINT32_MAX stays free as "none")
#define KO_MAX_DEAD_BYTES (1ull << 36)    // the dead words a call keeps in HBM (8 V_g bytes per chunk)
#define KO_MAX_SET_NODES 0xFFFFFFFFull    // nodes named by the sets of one call
#define KO_LDS_MAX 81920u                 // largest LDS image k_ko_lds takes: two workgroups per CU
#define KO_NO_OFF (~0ull)
#define KO_TIER_LDS 0u
#define KO_TIER_GLOB 1u

KO_HD static inline uint32_t ko_align(uint32_t b) { return (b + 15u) & ~15u; }

// k_ko_lds's image of a graph of V nodes, E edges and L Kahn levels: a u64 dead word per node, the forward
// rows, the Kahn order and the level offsets as u16, and a rule bit per node.
KO_HD static inline uint32_t knock_lds_bytes(uint32_t V, uint32_t E, uint32_t L) {
  return ko_align(8u * V) + ko_align(2u * (V + 1u)) + ko_align(2u * E) + ko_align(2u * V) + ko_align(2u * (L + 1u)) +
         ko_align(8u * ((V + 63u) / 64u));
}

// The LDS tier: u16 rows (V < 65536, E <= 65535: a row pointer is at most E) and an image of at most lds_max
// bytes (option knock_lds_max; 0: no graph).
static inline bool lds_fits(uint64_t V, uint64_t E, uint64_t L, uint32_t lds_max) {
  if (!lds_max || V >= 65536 || E > 65535 || L > V) return false;
  return knock_lds_bytes((uint32_t)V, (uint32_t)E, (uint32_t)L) <= lds_max;
}

// One listed graph of a call (leaves mode: a list position; sets mode: the one graph).
struct GraphIn {
  uint32_t graph;  // 2r + cond
  uint64_t V;      // its nodes
  uint64_t n;      // its hypotheses
  bool lds;        // lds_fits
};

// One chunk, as the kernels read it (two 16-byte loads).
struct Chunk {
  uint32_t graph;  // the graph the chunk's hypotheses are on
  uint32_t first;  // its first hypothesis (index into the call's rows)
  uint32_t n;      // 1..64 hypotheses
  uint32_t tier;   // KO_TIER_*
  uint64_t moff;   // first u64 of the chunk's dead words (KO_NO_OFF: an LDS chunk of a call without masks)
  uint32_t slot;   // the list position
  uint32_t pad;
};
static_assert(sizeof(Chunk) == 32, "two 16-byte loads");

// dead words of one chunk: a word per node, whole 16-byte pairs
KO_HD static inline uint64_t dead_words(uint64_t V) { return (V + 1) & ~1ull; }

enum Limit { LIMIT_OK = 0, LIMIT_HYPS = 1, LIMIT_DEAD = 2 };

struct Totals {
  uint64_t n_hyp = 0, n_chunks = 0, dead = 0;  // dead: u64 words kept in HBM
  Limit limit = LIMIT_OK;
};

// The call's totals and limits, without building the table.  With masks every chunk keeps its dead words; without,
// the global tier's chunks alone (their sweep runs in them).  Sums saturate instead of wrapping.
static inline Totals totals(const GraphIn *in, size_t n, bool masks) {
  Totals t;
  for (size_t i = 0; i < n; i++) {
    const uint64_t ck = in[i].n / KO_CHUNK + (in[i].n % KO_CHUNK != 0);
    t.n_hyp = t.n_hyp + in[i].n < t.n_hyp ? ~0ull : t.n_hyp + in[i].n;
    t.n_chunks += ck;
    if (masks || !in[i].lds) {
      const uint64_t w = dead_words(in[i].V);
      const uint64_t add = (w && ck > (~0ull - t.dead) / w) ? ~0ull - t.dead : ck * w;
      t.dead += add;
    }
  }
  if (t.n_hyp > KO_MAX_HYPS) t.limit = LIMIT_HYPS;
  else if (t.dead > KO_MAX_DEAD_BYTES / 8) t.limit = LIMIT_DEAD;
  return t;
}

struct Table {
  std::vector<Chunk> chunk;
  std::vector<uint64_t> first;  // per listed graph: its first hypothesis
  std::vector<uint32_t> count;  // ... and how many
  std::vector<uint32_t> sel;    // chunk indices: the LDS tier's, then the global tier's
  uint32_t n_lds = 0, n_glob = 0;
  Totals tot;
};

// The chunk table of a call within its limits (totals() said LIMIT_OK): graphs in list order, a graph's chunks
// in hypothesis order; a graph without hypotheses has no chunk and an empty range.
static inline Table chunk_table(const GraphIn *in, size_t n, bool masks) {
  Table t;
  t.tot = totals(in, n, masks);
  if (t.tot.limit != LIMIT_OK) return t;
  t.chunk.reserve(t.tot.n_chunks);
  t.first.resize(n);
  t.count.resize(n);
  uint64_t hyp = 0, off = 0;
  for (size_t i = 0; i < n; i++) {
    t.first[i] = hyp;
    t.count[i] = (uint32_t)in[i].n;
    for (uint64_t k = 0; k < in[i].n; k += KO_CHUNK) {
      Chunk c{};
      c.graph = in[i].graph;
      c.first = (uint32_t)(hyp + k);
      c.n = (uint32_t)(in[i].n - k < KO_CHUNK ? in[i].n - k : KO_CHUNK);
      c.tier = in[i].lds ? KO_TIER_LDS : KO_TIER_GLOB;
      c.moff = KO_NO_OFF;
      if (masks || !in[i].lds) {
        c.moff = off;
        off += dead_words(in[i].V);
      }
      c.slot = (uint32_t)i;
      t.chunk.push_back(c);
    }
    hyp += in[i].n;
  }
  for (uint32_t tier = KO_TIER_LDS; tier <= KO_TIER_GLOB; tier++)
    for (size_t k = 0; k < t.chunk.size(); k++)
      if (t.chunk[k].tier == tier) t.sel.push_back((uint32_t)k);
  for (const Chunk &c : t.chunk) (c.tier == KO_TIER_LDS ? t.n_lds : t.n_glob)++;
  return t;
}

// the chunk of hypothesis h (h < n_hyp)
static inline size_t chunk_of(const Table &t, uint64_t h) {
  size_t lo = 0, hi = t.chunk.size();
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (t.chunk[mid].first <= h) lo = mid;
    else hi = mid;
  }
  return lo;
}

enum SetCheck { SET_OK = 0, SET_NONMONOTONE = 1, SET_NODE = 2, SET_LIMIT = 3 };

// The explicit sets of nemo_knockout_sets: set s is set_nodes[set_off[s] .. set_off[s + 1]).  set_off must not
// decrease, the sets may name at most KO_MAX_SET_NODES nodes in all, and every node must be < V.  *where is
// the set (SET_NONMONOTONE) or the position in set_nodes (SET_NODE) of the first offence.
static inline SetCheck check_sets(const uint64_t *set_off, const uint32_t *set_nodes, size_t n_sets, uint64_t V,
                                  uint64_t *where) {
  if (!n_sets) return SET_OK;
  for (size_t s = 0; s < n_sets; s++)
    if (set_off[s + 1] < set_off[s]) {
      if (where) *where = s;
      return SET_NONMONOTONE;
    }
  if (set_off[n_sets] - set_off[0] > KO_MAX_SET_NODES) return SET_LIMIT;
  for (uint64_t k = set_off[0]; k < set_off[n_sets]; k++)
    if (set_nodes[k] >= V) {
      if (where) *where = k;
      return SET_NODE;
    }
  return SET_OK;
}

}  // namespace knock
