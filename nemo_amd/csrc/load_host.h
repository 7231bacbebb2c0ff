// load_host.h — the parts of nemo_load_corpus that touch no device: the argument checks with the
// host view, and run 0's goal-label tables.  Apart from api.hip, tools/load_host_check.cpp runs
// them under the host sanitizers.
#pragma once
#include "ctx.h"

// Argument checks and the host view of `in` (CorpusState's first block).  Allocates nothing on
// the device; a failure leaves the view partly written and `loaded` false.
inline int load_validate(nemo_ctx *c, const nemo_corpus *in) {
  CorpusState &s = c->cs;
  if (in->n_tables > NEMO_MAX_TABLES)
    return fail(c, NEMO_ERR_LIMIT, "%u tables exceed NEMO_MAX_TABLES (%u)", in->n_tables, NEMO_MAX_TABLES);
  if (!in->iteration || !in->node_off || !in->edge_off || (!in->node_word && in->n_runs))
    return fail(c, NEMO_ERR_INVALID, "corpus arrays missing");
  s.n_runs = in->n_runs;
  s.G = 2 * in->n_runs;
  s.T = in->n_tables;
  s.W = (in->n_tables + 31) / 32;
  s.table_pre = in->table_pre;
  s.table_post = in->table_post;
  s.iteration.assign(in->iteration, in->iteration + in->n_runs);
  s.owned.assign(in->n_runs, 1);
  if (in->owned)
    for (uint32_t r = 0; r < in->n_runs; r++) s.owned[r] = in->owned[r] ? 1 : 0;
  s.node_off.assign(in->node_off, in->node_off + s.G + 1);
  s.edge_off.assign(in->edge_off, in->edge_off + s.G + 1);
  s.V = s.node_off[s.G];
  s.E = s.edge_off[s.G];
  s.postV = s.postE = 0;
  for (uint32_t g = 1; g < s.G; g += 2) {
    s.postV += (double)s.nv(g);
    s.postE += (double)s.ne(g);
  }
  s.it2run.clear();
  s.run0 = -1;
  for (uint32_t r = 0; r < s.n_runs; r++) {
    if (s.it2run.count(s.iteration[r]))
      return fail(c, NEMO_ERR_INVALID, "duplicate run iteration %u", s.iteration[r]);
    s.it2run[s.iteration[r]] = r;
    if (s.iteration[r] == 0) s.run0 = (int32_t)r;
  }
  for (uint32_t g = 0; g < s.G; g++) {
    if (s.node_off[g + 1] < s.node_off[g] || s.edge_off[g + 1] < s.edge_off[g])
      return fail(c, NEMO_ERR_INVALID, "offsets not monotone at graph %u", g);
    if (s.nv(g) >= 0xFFFFFFF0ull || s.ne(g) >= 0xFFFFFFF0ull)
      return fail(c, NEMO_ERR_LIMIT, "graph %u exceeds 2^32 nodes/edges", g);
  }
  if (s.node_off[0] != 0 || s.edge_off[0] != 0) return fail(c, NEMO_ERR_INVALID, "offsets must start at 0");
  s.has_rank = in->id_rank != nullptr;
  s.pairs_wide = false;
  for (uint32_t g = 0; g < s.G; g++) s.pairs_wide |= s.nv(g) >= 65536;
  return NEMO_OK;
}

// Run 0's post goal labels for the diff's failGoals lookup.
struct R0Tables {
  std::vector<uint32_t> l, ix;       // the labels, sorted, and each one's node (index within g0)
  std::vector<uint32_t> hkey, hval;  // label + 1 -> first sorted entry; hkey.size() is a power of two
  std::vector<uint32_t> dense;       // label -> (first sorted entry << 4 | min(count, 15)); empty: no dense table
};

inline R0Tables r0_tables(const CorpusState &s, const nemo_corpus *in) {
  R0Tables t;
  const uint32_t g0 = 2 * s.run0 + 1;
  std::vector<std::pair<uint32_t, uint32_t>> lab;
  for (uint64_t v = s.node_off[g0]; v < s.node_off[g0 + 1]; v++)
    if (!(in->node_word[v] & NEMO_NODE_RULE)) lab.push_back({in->label[v], (uint32_t)(v - s.node_off[g0])});
  std::sort(lab.begin(), lab.end());
  std::vector<uint32_t> &l = t.l;
  l.resize(lab.size());
  t.ix.resize(lab.size());
  for (size_t i = 0; i < lab.size(); i++) {
    l[i] = lab[i].first;
    t.ix[i] = lab[i].second;
  }
  // label -> first sorted entry, open-addressed at load factor <= 1/2, so a
  // lookup is one or two independent probes instead of a binary search
  uint32_t hcap = 16;
  while (hcap < 2 * lab.size()) hcap <<= 1;
  t.hkey.assign(hcap, 0u);
  t.hval.assign(hcap, 0u);
  for (size_t i = 0; i < l.size(); i++) {
    if (i && l[i] == l[i - 1]) continue;
    uint32_t h = hash_label(l[i]) & (hcap - 1);
    while (t.hkey[h]) h = (h + 1) & (hcap - 1);
    t.hkey[h] = l[i] + 1u;
    t.hval[h] = (uint32_t)i;
  }
  // the same as a dense table over the label ids up to run 0's largest goal label (a source label
  // past it is no run-0 goal label), when that is at most 256M entries: one load per source goal
  // instead of a probe sequence
  const uint64_t nlab = l.empty() ? 0 : (uint64_t)l.back() + 1;
  if (nlab && nlab <= (1ull << 28)) {
    t.dense.assign(nlab, NEMO_NONE);
    for (size_t i = 0; i < l.size();) {
      size_t j = i;
      while (j < l.size() && l[j] == l[i]) j++;
      t.dense[l[i]] = (uint32_t)(i << 4) | (uint32_t)std::min<size_t>(j - i, 15);
      i = j;
    }
  }
  return t;
}
