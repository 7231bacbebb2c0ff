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

}  // namespace gdedup
