// lin_run.h — lin_api.h's level loop and the keys' way to the host as two functions, for a search that lives in a
// translation unit of its own beside the two lineage cut searches (api_lrepair.hip: nemo_lineage_repair_sets /
// nemo_lineage_repairs).  The loop stays lin_api.h's, once: api_lineage.hip defines the two functions over lin_levels and
// lin_sorted_keys, with the call's hooks as std::function; what the hooks are and when they run is stated there.
#pragma once
#include <functional>
#include <vector>

#include "knock_api.h"

struct LinRun {
  const char *who, *shorten;   // the calling entry point's name and what its messages tell the caller to shorten
  LinBufs *bufs;               // the call's own buffers, bufs->ctr in place
  Pinned<uint64_t> *h;         // ... pinned buffer (8 elements at least)
  hipEvent_t ev;               // ... and event
  nemo::LinArgs *a;            // the level as the kernels read it: graph, cand, lds_total, region, region_words are the caller's
  uint64_t K;
  uint32_t max_size;
  uint64_t *stats;             // [18] per size 0..8: sets evaluated, sets found
  std::function<int(uint64_t n_front, uint32_t d)> level_limit;
  std::function<int(int pass, double *bytes, double *ops)> evaluate;
  std::function<uint64_t(uint64_t n_front, uint32_t d)> emit_bound;
};

// lin_levels over r (no column, nothing sized by the level); *n_found: the sets in r.bufs->cuts at the end
int lin_levels_run(nemo_ctx *c, const LinRun &r, double *bytes, double *ops, uint64_t *n_found);
// lin_sorted_keys: the n keys of b.cuts as the device holds them, and the rows' order (row i is keys[order[i]])
int lin_sorted_run(nemo_ctx *c, const LinBufs &b, Pinned<uint64_t> &h, hipEvent_t ev, uint64_t n, std::vector<lin::Key> *keys,
                   std::vector<uint32_t> *order);
