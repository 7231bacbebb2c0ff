// gdedup_host.h — the host side of the duplicate-graph classes (k_gdedup.hip) as pure
// functions: hashes in, candidate pairs out, verdicts in (dclass::Refiner, the bucket-and-confirm
// rounds of nemo_diff_classes), then the lists the per-graph kernels and the replicate kernel run
// over.  No HIP and no context, so tools/gdedup_host_check.cpp drives it under the host sanitizers.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "dclass_host.h"

namespace gdedup {

// What a load keeps of its classes.  A graph that is `eligible` and whose content equals an earlier
// eligible graph's is a duplicate; every other graph is its own representative.
struct Plan {
  std::vector<uint32_t> rep;    // [G] graph -> the lowest-numbered graph of its class (itself: a representative)
  std::vector<uint32_t> list;   // the representatives, ascending: what the per-graph kernels run over
  std::vector<uint32_t> pairs;  // (dup, rep) per duplicate, sorted by rep then dup: the replicate kernel's work
  uint32_t classes = 0;         // distinct contents among the eligible graphs
  uint64_t dup_nodes = 0;       // nodes of the duplicates
};

// rep: Refiner::rep() over all G graphs (classes by content; the content covers V, E and the
// parity, so a class is all pre or all post graphs of one size).  eligible[g]: the graph may be
// deduplicated (the same for every graph of a class, as it depends on the size alone).
static inline Plan plan(const std::vector<uint32_t> &rep, const std::vector<uint8_t> &eligible, const uint64_t *node_off) {
  const uint32_t G = (uint32_t)rep.size();
  Plan p;
  p.rep.resize(G);
  for (uint32_t g = 0; g < G; g++) {
    const uint32_t r = eligible[g] && rep[g] < g && eligible[rep[g]] && ((rep[g] ^ g) & 1u) == 0u ? rep[g] : g;
    p.rep[g] = r;
    if (r == g) {
      p.list.push_back(g);
      p.classes += eligible[g] ? 1u : 0u;
    } else {
      p.pairs.push_back(r);  // (rep, dup) for the sort below
      p.pairs.push_back(g);
      p.dup_nodes += node_off[g + 1] - node_off[g];
    }
  }
  const size_t n = p.pairs.size() / 2;
  std::vector<std::pair<uint32_t, uint32_t>> v(n);
  for (size_t k = 0; k < n; k++) v[k] = {p.pairs[2 * k], p.pairs[2 * k + 1]};
  std::sort(v.begin(), v.end());
  for (size_t k = 0; k < n; k++) {
    p.pairs[2 * k] = v[k].second;  // dup
    p.pairs[2 * k + 1] = v[k].first;  // rep
  }
  return p;
}

// A pull over one graph per class: slot k compacts graph list[k], and graph g is handed the region of
// slot map[g].  A graph that is `apart` (the same for every graph of a class: it depends on the size
// alone) keeps a slot of its own, as the graphs outside a kernel's tier do everywhere else; any other
// takes its representative's.  map[g] <= g (a representative is the lowest graph of its class and the
// list ascends), which is what an in-place expansion of the slot tables from the last graph down needs.
struct PullPlan {
  std::vector<uint32_t> list, map;
};
static inline PullPlan pull_plan(const std::vector<uint32_t> &rep, const std::vector<uint8_t> &apart) {
  const uint32_t G = (uint32_t)rep.size();
  PullPlan p;
  p.map.resize(G);
  std::vector<uint32_t> at(G, 0);
  for (uint32_t g = 0; g < G; g++) {
    if (rep[g] == g || apart[g]) {
      at[g] = (uint32_t)p.list.size();
      p.list.push_back(g);
    }
    p.map[g] = at[apart[g] ? g : rep[g]];
  }
  return p;
}

// Run classes: runs r and r' are of one class iff their pre graphs are of one graph class and their
// post graphs are (rep[2r] == rep[2r'] and rep[2r + 1] == rep[2r' + 1]).  What a per-run kernel
// computes from the two graphs alone (k_proto_lds) is then the same for both.
struct RunPlan {
  std::vector<uint32_t> rep;    // [n_runs] run -> the lowest-numbered run of its class
  std::vector<uint32_t> list;   // the representative runs, ascending
  std::vector<uint32_t> pairs;  // (dup, rep) per duplicate run, sorted by rep then dup
};

// rep: Plan::rep over the 2 n_runs graphs
static inline RunPlan run_plan(const std::vector<uint32_t> &rep) {
  const uint32_t n = (uint32_t)(rep.size() / 2);
  RunPlan p;
  p.rep.resize(n);
  std::vector<std::pair<uint64_t, uint32_t>> key(n);  // ((pre class, post class), run)
  for (uint32_t r = 0; r < n; r++) key[r] = {((uint64_t)rep[2 * r] << 32) | rep[2 * r + 1], r};
  std::sort(key.begin(), key.end());
  std::vector<std::pair<uint32_t, uint32_t>> v;  // (rep, dup)
  for (uint32_t k = 0, first = 0; k < n; k++) {
    if (key[k].first != key[first].first) first = k;
    p.rep[key[k].second] = key[first].second;  // the lowest run of the key: runs ascend within a key
    if (k != first) v.push_back({key[first].second, key[k].second});
  }
  for (uint32_t r = 0; r < n; r++)
    if (p.rep[r] == r) p.list.push_back(r);
  std::sort(v.begin(), v.end());
  for (auto &x : v) {
    p.pairs.push_back(x.second);
    p.pairs.push_back(x.first);
  }
  return p;
}

}  // namespace gdedup
