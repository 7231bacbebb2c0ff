// dclass_host.h — the host side of nemo_diff_classes as pure functions: hashes in, candidate lists
// out, verdicts in, class_of / classes out.  No HIP and no context, so tools/dclass_host_check.cpp
// drives it under the host sanitizers; api_diff.hip and node.hip run the rounds with it.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/nemohip.h"

namespace dclass {

struct Hash {
  uint64_t lo = 0, hi = 0;
};

// the low `bits` bits of a hash (option class_hash_bits: 0 = every mask collides)
static inline Hash low_bits(Hash h, int bits) {
  if (bits >= 128) return h;
  if (bits <= 0) return Hash{};
  if (bits >= 64) {
    if (bits > 64) h.hi &= ~0ull >> (128 - bits);
    else h.hi = 0;
    return h;
  }
  h.hi = 0;
  h.lo &= ~0ull >> (64 - bits);
  return h;
}

// Partition of n items (the distinct sources, in order of their first entry) into classes of
// identical rows.  Items are bucketed by hash; equality inside a bucket is decided by the caller's
// exact row comparisons, one round at a time: every bucket's smallest unresolved item becomes a
// class representative, the bucket's other unresolved items are compared with it, the unequal ones
// stay for the next round.  Equal rows have equal hashes, so no class spans two buckets.
class Refiner {
 public:
  Refiner(const Hash *h, uint32_t n, int bits) : rep_(n, 0) {
    std::vector<Hash> key(n);
    for (uint32_t i = 0; i < n; i++) key[i] = low_bits(h[i], bits);
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
      if (key[a].hi != key[b].hi) return key[a].hi < key[b].hi;
      if (key[a].lo != key[b].lo) return key[a].lo < key[b].lo;
      return a < b;
    });
    for (uint32_t i = 0; i < n; i++) {
      const bool same = i && key[order[i]].hi == key[order[i - 1]].hi && key[order[i]].lo == key[order[i - 1]].lo;
      if (!same) open_.emplace_back();
      open_.back().push_back(order[i]);  // ascending inside a bucket
    }
  }
  // The next round's comparisons as (item, candidate) pairs, pairs[2k], pairs[2k + 1].  Returns false
  // once every item has its class; a round may need no comparison at all (pairs empty, returns true).
  bool next_round(std::vector<uint32_t> &pairs) {
    pairs.clear();
    bool any = false;
    for (auto &b : open_) {
      if (b.empty()) continue;
      any = true;
      rep_[b[0]] = b[0];
      for (size_t k = 1; k < b.size(); k++) {
        pairs.push_back(b[k]);
        pairs.push_back(b[0]);
      }
    }
    if (!any) open_.clear();
    rounds_ += any;
    return any;
  }
  // One verdict per pair of the last next_round, in its order: non-zero = the rows are equal.
  void verdicts(const uint8_t *v) {
    size_t k = 0;
    for (auto &b : open_) {
      if (b.empty()) continue;
      size_t left = 0;
      const uint32_t cand = b[0];
      for (size_t i = 1; i < b.size(); i++, k++) {
        if (v[k]) rep_[b[i]] = cand;
        else b[left++] = b[i];
      }
      b.resize(left);
    }
  }
  const std::vector<uint32_t> &rep() const { return rep_; }  // item -> its class's smallest item
  uint32_t rounds() const { return rounds_; }

 private:
  std::vector<std::vector<uint32_t>> open_;  // per bucket: the unresolved items
  std::vector<uint32_t> rep_;
  uint32_t rounds_ = 0;
};

// Entries from items: entry e's item is item_of[e]; item i's first entry is first_entry[i] (ascending
// in i) and its row has nodes[i] members.  Classes are numbered by their smallest entry.
static inline void finish(const std::vector<uint32_t> &rep, const uint32_t *item_of, uint32_t n_entries,
                          const uint32_t *first_entry, const uint32_t *nodes, std::vector<uint32_t> &class_of,
                          std::vector<nemo_diff_class> &classes) {
  std::vector<uint32_t> cid(rep.size(), 0);
  classes.clear();
  for (uint32_t i = 0; i < rep.size(); i++)
    if (rep[i] == i) {
      cid[i] = (uint32_t)classes.size();
      classes.push_back(nemo_diff_class{first_entry[i], 0u, nodes[i]});
    }
  class_of.assign(n_entries, 0);
  for (uint32_t e = 0; e < n_entries; e++) {
    class_of[e] = cid[rep[item_of[e]]];
    classes[class_of[e]].size++;
  }
}

}  // namespace dclass
