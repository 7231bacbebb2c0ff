// pairs_host.h — the host side of nemo_diffprov_pairs' label hash tables (k_sdiff.hip k_lab_hash;
// DESIGN.md §Pair diff) as pure functions: the call's `other` graphs in, the distinct graphs that
// need a table, each table's capacity and its place in the per-call region out.  No HIP and no
// context, so tools/pairs_host_check.cpp drives it under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <unordered_map>
#include <vector>

namespace pairs {

#define PAIRS_SHARED 0xFFFFFFFFu  // Plan::entry_tab: the entry probes the load's run-0 table
#define PAIRS_MIN_CAP 16u         // as the load's run-0 table (load_host.h r0_tables)

// Slots of the table of a graph of `nodes` nodes: the smallest power of two that is at least
// PAIRS_MIN_CAP and at least twice the nodes.  The nodes bound the goals and the goals bound the
// distinct labels, so the load factor is at most 1/2 and a probe sequence always meets an empty
// slot.  A multiple of four: a table is written and zeroed in 16-byte stores.
static inline uint64_t capacity(uint64_t nodes) {
  uint64_t cap = PAIRS_MIN_CAP;
  while (cap < 2 * nodes) cap <<= 1;
  return cap;
}

struct Plan {
  std::vector<uint32_t> tab_graph;  // [tables] the distinct `other` graphs that get a table, by first entry
  std::vector<uint64_t> tab_off;    // [tables + 1] first slot of each table in the region; [tables] = words
  std::vector<uint32_t> tab_mask;   // [tables] capacity - 1
  std::vector<uint32_t> entry_tab;  // [entries] the entry's table, or PAIRS_SHARED
  uint64_t words = 0;               // u32 slots of the region
  uint64_t nodes = 0;               // nodes of the hashed graphs (the kernel's reads: 8 bytes each)
  uint64_t max_cap = 0;             // the largest table
  bool ok = true;                   // false: a table would pass 2^32 slots (its mask has 32 bits)
};

// other_graph[e]: entry e's `other` post graph.  shared_graph: the graph whose table the load built
// (run 0's post graph), or a negative value when the corpus has no run 0: entries against it build
// nothing.  Tables are laid out back to back in first-entry order; every offset is a multiple of four.
static inline Plan plan(const uint32_t *other_graph, size_t n, const uint64_t *node_off, int64_t shared_graph) {
  Plan p;
  p.entry_tab.resize(n);
  p.tab_off.push_back(0);
  std::unordered_map<uint32_t, uint32_t> seen;
  for (size_t e = 0; e < n; e++) {
    const uint32_t g = other_graph[e];
    if (shared_graph >= 0 && (int64_t)g == shared_graph) {
      p.entry_tab[e] = PAIRS_SHARED;
      continue;
    }
    auto ins = seen.emplace(g, (uint32_t)p.tab_graph.size());
    if (ins.second) {
      const uint64_t v = node_off[g + 1] - node_off[g], cap = capacity(v);
      if (cap > (1ull << 32)) p.ok = false;
      p.tab_graph.push_back(g);
      p.tab_mask.push_back((uint32_t)(cap - 1));
      p.tab_off.push_back(p.tab_off.back() + cap);
      p.nodes += v;
      if (cap > p.max_cap) p.max_cap = cap;
    }
    p.entry_tab[e] = ins.first->second;
  }
  p.words = p.tab_off.back();
  return p;
}

}  // namespace pairs
