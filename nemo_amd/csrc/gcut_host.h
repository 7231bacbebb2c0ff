// gcut_host.h — the arithmetic of nemo_min_group_cuts (k_gcuts.hip; DESIGN.md §Minimal cut sets over fault events) as
// pure functions: the check of the groups (offsets, the forbidden label, the totals), the count of the distinct
// labels the groups name, the size of the label -> row table, and the sizes of a workgroup's hit list and region.
// The colex ranks and the round sizes are cut_host.h's, the hash, the work items and the offset check
// klabel_host.h's, the min_runs rule, the rounds' limits and the live list lcut_host.h's.  No HIP and no context, so
// tools/gcut_host_check.cpp drives it under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "cut_host.h"
#include "klabel_host.h"
#include "lcut_host.h"

namespace gcuts {

#define GC_MAX_LABELS KL_MAX_LABELS  // labels named by the groups of one call: an entry index is a u32 on the device
#define GC_NO_LABEL KL_NO_LABEL      // no legal label: label + 1 is the table key
// labels of one group: a chunk's sweep scans the lengths of the up to 3 x 64 groups of its sets in u32, and 192 x 2^24
// stays below 2^32
#define GC_MAX_GROUP (1ull << 24)
#define GC_MAX_LIST 0xFFFFFFFFull    // entries of a graph's hit list: an entry index is a u32 on the device

enum GroupCheck { GROUP_OK = 0, GROUP_NONMONOTONE = 1, GROUP_LABEL = 2, GROUP_LIMIT = 3, GROUP_SIZE = 4 };

// The groups of nemo_min_group_cuts: group k is group_labels[group_off[k] .. group_off[k + 1]).  The offsets are
// checked first (so a call past the label limit reads no label): they must not decrease, and the groups may name
// at most GC_MAX_LABELS labels in all and one group at most GC_MAX_GROUP; then every label must differ from
// GC_NO_LABEL.  *group: the group of the first offence (GROUP_NONMONOTONE: the first decreasing one, GROUP_SIZE: the
// first one too long), *where: the position in group_labels (GROUP_LABEL).
static inline GroupCheck check_groups(const uint64_t *group_off, const uint32_t *group_labels, size_t n_groups, uint64_t *group,
                                      uint64_t *where) {
  switch (klabel::check_offsets(group_off, n_groups, group)) {
    case klabel::SET_NONMONOTONE:
      return GROUP_NONMONOTONE;
    case klabel::SET_LIMIT:
      return GROUP_LIMIT;
    default:
      break;
  }
  for (size_t k = 0; k < n_groups; k++)
    if (group_off[k + 1] - group_off[k] > GC_MAX_GROUP) {
      if (group) *group = k;
      return GROUP_SIZE;
    }
  for (size_t k = 0; k < n_groups; k++)
    for (uint64_t e = group_off[k]; e < group_off[k + 1]; e++)
      if (group_labels[e] == GC_NO_LABEL) {
        if (group) *group = k;
        if (where) *where = e;
        return GROUP_LABEL;
      }
  return GROUP_OK;
}

// labels the groups name in all (checked offsets)
static inline uint64_t named(const uint64_t *group_off, size_t n_groups) { return n_groups ? group_off[n_groups] - group_off[0] : 0; }

// The offsets as the device reads them: u32, from the first group's (checked groups: the total fits).
static inline std::vector<uint32_t> offsets32(const uint64_t *group_off, size_t n_groups) {
  std::vector<uint32_t> off(n_groups + 1, 0u);
  for (size_t k = 0; k <= n_groups && n_groups; k++) off[k] = (uint32_t)(group_off[k] - group_off[0]);
  return off;
}

// D: the distinct labels among the named ones (a label named twice, in one group or in two, is one row of a
// graph's hit list).  The host counts them before the device reads any label: D bounds a workgroup's region.
static inline uint64_t distinct_labels(const uint64_t *group_off, const uint32_t *group_labels, size_t n_groups) {
  if (!named(group_off, n_groups)) return 0;
  std::vector<uint32_t> l(group_labels + group_off[0], group_labels + group_off[n_groups]);
  std::sort(l.begin(), l.end());
  return (uint64_t)(std::unique(l.begin(), l.end()) - l.begin());
}

// slots of the call's label -> row table (d distinct labels; load <= 1/2)
static inline uint64_t table_slots(uint64_t d) { return klabel::table_slots(d); }

// A graph's hit list: d + 1 row offsets, then at most V nodes, u32 each (a node carries one label: one row), so
// O(D + V) whatever the groups share; `head` of them stay in LDS behind the image, the others follow `dead` dead
// words in the workgroup's region (u64 words).  lcut_host.h's layout with a row per distinct label.
static inline uint64_t list_entries(uint64_t d, uint64_t V) { return lcuts::list_entries(d, V); }
static inline bool list_fits(uint64_t d, uint64_t V) { return list_entries(d, V) <= GC_MAX_LIST; }
static inline uint64_t region_words(uint64_t dead, uint64_t entries, uint64_t head) { return lcuts::region_words(dead, entries, head); }

}  // namespace gcuts
