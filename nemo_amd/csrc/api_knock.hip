// api_knock.hip — nemo_knockout_leaves, nemo_knockout_sets and their fetches (k_knock.hip).
#include "knock_api.h"

namespace {

// what every knock-out entry point checks first; leaves the device set and the graphs whole
int ko_enter(nemo_ctx *c, const char *who, int cond, uint32_t flags) {
  CorpusState &cs = c->cs;
  if (!cs.loaded) return fail(c, NEMO_ERR_STATE, "%s without a loaded corpus (the last load failed?)", who);
  cs.ko_done = false;
  cs.ko_masks = false;
  if (cond != 0 && cond != 1) return fail(c, NEMO_ERR_INVALID, "%s: cond must be 0 (pre) or 1 (post)", who);
  if (flags & ~NEMO_KO_MASKS) return fail(c, NEMO_ERR_INVALID, "%s: unknown flags %#x", who, flags);
  HIPCHK(c, hipSetDevice(c->device));
  if (int rw = ensure_whole(c)) return rw;  // may read any graph's build outputs
  return ensure_load_checked(c);
}

int ko_limit(nemo_ctx *c, const char *who, const knock::Totals &t) {
  if (t.limit == knock::LIMIT_HYPS)
    return fail(c, NEMO_ERR_LIMIT, "%s: %llu hypotheses exceed 2^32 - 2 in one call: tile the call", who,
                (unsigned long long)t.n_hyp);
  return fail(c, NEMO_ERR_LIMIT,
              "%s: the dead words of %llu chunks (8 bytes per node and chunk of 64 hypotheses) exceed 2^36 bytes: tile the call",
              who, (unsigned long long)t.n_chunks);
}

// The five per-hypothesis buffers grow as one group (ctx.h's grow_group), each to the largest request so far, in
// this order.  The leaves are none when every set is empty, the dead words when no chunk keeps them: one element
// then, so that such a call finds the group grown.
int ko_buffers(nemo_ctx *c, uint64_t n_leaf, uint64_t n_setoff, const knock::Totals &tot) {
  CorpusState &cs = c->cs;
  const uint64_t need[5] = {std::max<uint64_t>(n_leaf, 1), tot.n_chunks + (tot.n_chunks + 7) / 8, n_setoff, 5 * tot.n_hyp,
                            std::max<uint64_t>(tot.dead, 1)};
  return grow_group(c, need, cs.d_koleaf, cs.d_kochunk, cs.d_koset, cs.d_korows, cs.d_kodead);
}

// The sweep of a call whose table, leaves / sets and buffers are in place: both tiers, the rows to pinned
// memory, and the wait for them.  set_nodes: the nodes the sets name in all (sets mode).
int ko_sweep(nemo_ctx *c, nemo::KnockArgs &a, const std::vector<knock::GraphIn> &in, const std::vector<uint32_t> &levels,
             uint64_t set_nodes, GroupTimer &timer, double bytes_before) {
  CorpusState &cs = c->cs;
  const knock::Table &t = cs.ko_tab;
  hipStream_t s = c->stream;
  const uint64_t nck = t.chunk.size();
  HIPCHK(c, hipMemcpyAsync(cs.d_kochunk.p, t.chunk.data(), nck * sizeof(knock::Chunk), hipMemcpyHostToDevice, s));
  uint32_t *d_sel = reinterpret_cast<uint32_t *>(cs.d_kochunk.p + nck);
  HIPCHK(c, hipMemcpyAsync(d_sel, t.sel.data(), t.sel.size() * 4, hipMemcpyHostToDevice, s));
  a.chunk = reinterpret_cast<const uint4 *>(cs.d_kochunk.p);
  a.dead = cs.d_kodead.p;
  a.rows = cs.d_korows.p;
  a.masks = cs.ko_masks ? 1u : 0u;
  // the byte model per (graph, chunk): the image read (row pointers 4 (V + 1), children 4 E, Kahn order 4 V,
  // level offsets 4 (L + 1), node words 4 V), the chunk's row and seeds, its rows, and 8 V when its words are kept
  double b_tier[2] = {0, 0}, ops[2] = {0, 0};
  uint32_t lds_bytes = 0;
  for (size_t i = 0; i < in.size(); i++) {
    const double V = (double)in[i].V, E = (double)cs.ne(in[i].graph), L = (double)levels[i];
    const double ck = (double)((in[i].n + KO_CHUNK - 1) / KO_CHUNK);
    const int tier = in[i].lds ? 0 : 1;
    b_tier[tier] += ck * (4.0 * E + 12.0 * V + 4.0 * L + 8.0 + 32.0) + 24.0 * (double)in[i].n +
                    ((cs.ko_masks || !in[i].lds) ? ck * 8.0 * V : 0.0);
    ops[tier] += ck * E;
    if (in[i].lds && in[i].n)
      lds_bytes = std::max(lds_bytes, knock::knock_lds_bytes((uint32_t)in[i].V, (uint32_t)cs.ne(in[i].graph), levels[i]));
  }
  if (a.set_off) b_tier[in[0].lds ? 0 : 1] += 4.0 * (double)set_nodes + 4.0 * (double)t.tot.n_hyp;
  int rc;
  a.sel = d_sel;
  if (t.n_lds && (rc = timed(c, "k_ko_lds", b_tier[0], ops[0], [&] { nemo::launch_ko_lds(cs.dc, a, t.n_lds, lds_bytes, s); })))
    return rc;
  a.sel = d_sel + t.n_lds;
  if (t.n_glob && (rc = timed(c, "k_ko_glob", b_tier[1], ops[1], [&] { nemo::launch_ko_glob(cs.dc, a, t.n_glob, s); })))
    return rc;
  timer.done(bytes_before + b_tier[0] + b_tier[1], ops[0] + ops[1]);
  nemo::launch_to_host(c->h_knock.p, cs.d_korows.p, 20 * t.tot.n_hyp, s);  // the rows to pinned memory
  if ((rc = wait_copied(c, c->ev_knock))) return rc;
  cs.ko_done = true;
  return NEMO_OK;
}

}  // namespace

extern "C" {

// One hypothesis per sink goal of every listed graph.  k_ko_leaves counts them, the host reads the counts and
// the graphs' Kahn level counts in one blocking round trip (as nemo_diff_classes reads its hashes) and makes
// the chunk table; k_ko_leaves then lists the sink goals and the two tiers sweep.  The state is the call's own.
int nemo_knockout_leaves(nemo_ctx *c, const uint32_t *iters, size_t n, int cond, uint32_t flags) {
  if (c && c->node)
    return fail(c, NEMO_ERR_STATE, "nemo_knockout_leaves: single-device contexts only (a node context does not fan it out)");
  if (!c || (!iters && n)) return NEMO_ERR_INVALID;
  CorpusState &cs = c->cs;
  int rc;
  if ((rc = ko_enter(c, "nemo_knockout_leaves", cond, flags))) return rc;
  std::vector<uint32_t> &desc = cs.ko_desc;  // [n] graphs | [n + 1] first hypotheses
  desc.assign(2 * n + 1, 0u);
  for (size_t i = 0; i < n; i++) {
    uint32_t r;
    if ((rc = run_index(c, iters[i], &r))) return rc;
    desc[i] = 2 * r + (uint32_t)cond;
  }
  cs.ko_masks = (flags & NEMO_KO_MASKS) != 0;
  if (n == 0) {  // zero hypotheses
    cs.ko_tab = knock::Table{};
    cs.ko_done = true;
    return NEMO_OK;
  }
  if (n > KO_MAX_HYPS) return fail(c, NEMO_ERR_LIMIT, "nemo_knockout_leaves: %zu listed runs: tile the call", n);
  if ((rc = ensure_event(c, &c->ev_knock))) return rc;
  if ((rc = c->h_knock.grow(c, 2 * (uint64_t)n))) return rc;
  hipStream_t s = c->stream;
  GroupTimer timer(c, "k_knock");
  if (4 * (uint64_t)n + 1 > cs.d_kocnt.cap || !cs.d_kocnt.p) {
    HIPCHK(c, hipStreamSynchronize(s));
    if ((rc = cs.d_kocnt.grow(c, 4 * (uint64_t)n + 1))) return rc;
  }
  HIPCHK(c, hipMemcpyAsync(cs.d_kocnt.p, desc.data(), n * 4, hipMemcpyHostToDevice, s));
  nemo::KnockArgs a{};
  a.list = cs.d_kocnt.p;
  a.loff = cs.d_kocnt.p + n;
  a.cnt = cs.d_kocnt.p + 2 * n + 1;
  a.n_list = (uint32_t)n;
  double nodes = 0;
  for (size_t i = 0; i < n; i++) nodes += (double)cs.nv(desc[i]);
  const double b_leaves = 8.0 * nodes + 12.0 * (double)n;  // node word + row pointer of every node; the counts
  if ((rc = timed(c, "k_ko_leaves", b_leaves, 0, [&] { nemo::launch_ko_leaves(cs.dc, a, false, s); }))) return rc;
  nemo::launch_to_host(c->h_knock.p, a.cnt, 8 * (uint64_t)n, s);
  if ((rc = wait_copied(c, c->ev_knock))) return rc;
  std::vector<knock::GraphIn> in(n);
  std::vector<uint32_t> levels(n);
  for (size_t i = 0; i < n; i++) {
    const uint32_t g = desc[i];
    levels[i] = c->h_knock.p[2 * i + 1];
    in[i] = {g, cs.nv(g), c->h_knock.p[2 * i], knock::lds_fits(cs.nv(g), cs.ne(g), levels[i], c->opt.knock_lds_max)};
  }
  const knock::Totals tot = knock::totals(in.data(), n, cs.ko_masks);
  if (tot.limit != knock::LIMIT_OK) return ko_limit(c, "nemo_knockout_leaves", tot);
  cs.ko_tab = knock::chunk_table(in.data(), n, cs.ko_masks);
  const knock::Table &t = cs.ko_tab;
  for (size_t i = 0; i < n; i++) desc[n + i] = (uint32_t)t.first[i];
  desc[2 * n] = (uint32_t)tot.n_hyp;
  if (tot.n_hyp == 0) {  // no listed graph has a sink goal
    timer.done(b_leaves, 0);
    cs.ko_done = true;
    return NEMO_OK;
  }
  if ((rc = c->h_knock.grow(c, 5 * tot.n_hyp))) return rc;
  if ((rc = ko_buffers(c, tot.n_hyp, 1, tot))) return rc;
  HIPCHK(c, hipMemcpyAsync(cs.d_kocnt.p + n, desc.data() + n, (n + 1) * 4, hipMemcpyHostToDevice, s));
  a.leaf = cs.d_koleaf.p;
  a.set_off = nullptr;
  if ((rc = timed(c, "k_ko_leaves", b_leaves + 4.0 * (double)tot.n_hyp, 0, [&] { nemo::launch_ko_leaves(cs.dc, a, true, s); })))
    return rc;
  return ko_sweep(c, a, in, levels, 0, timer, 2.0 * b_leaves + 4.0 * (double)tot.n_hyp);
}

// Explicit hypotheses on one graph.  The sets are checked on the host (knock_host.h); the graph's Kahn level
// count comes back in one blocking round trip, for the tier.
int nemo_knockout_sets(nemo_ctx *c, uint32_t iteration, int cond, const uint64_t *set_off, const uint32_t *set_nodes,
                       size_t n_sets, uint32_t flags) {
  if (c && c->node)
    return fail(c, NEMO_ERR_STATE, "nemo_knockout_sets: single-device contexts only (a node context does not fan it out)");
  if (!c || (!set_off && n_sets)) return NEMO_ERR_INVALID;
  CorpusState &cs = c->cs;
  int rc;
  if ((rc = ko_enter(c, "nemo_knockout_sets", cond, flags))) return rc;
  uint32_t r;
  if ((rc = run_index(c, iteration, &r))) return rc;
  const uint32_t g = 2 * r + (uint32_t)cond;
  const uint64_t V = cs.nv(g);
  if (n_sets && set_off[n_sets] > set_off[0] && !set_nodes) return NEMO_ERR_INVALID;
  uint64_t where = 0;
  switch (knock::check_sets(set_off, set_nodes, n_sets, V, &where)) {
    case knock::SET_NONMONOTONE:
      return fail(c, NEMO_ERR_INVALID, "nemo_knockout_sets: set_off decreases at set %llu", (unsigned long long)where);
    case knock::SET_NODE:
      return fail(c, NEMO_ERR_INVALID, "nemo_knockout_sets: node %u at position %llu is out of range (%llu nodes)",
                  set_nodes[where], (unsigned long long)where, (unsigned long long)V);
    case knock::SET_LIMIT:
      return fail(c, NEMO_ERR_LIMIT, "nemo_knockout_sets: the sets name more than 2^32 - 1 nodes: tile the call");
    default:
      break;
  }
  cs.ko_masks = (flags & NEMO_KO_MASKS) != 0;
  if (n_sets == 0) {  // zero hypotheses
    cs.ko_tab = knock::Table{};
    cs.ko_done = true;
    return NEMO_OK;
  }
  if (n_sets > KO_MAX_HYPS) {
    knock::Totals t;
    t.n_hyp = n_sets;
    t.limit = knock::LIMIT_HYPS;
    return ko_limit(c, "nemo_knockout_sets", t);
  }
  if ((rc = ensure_event(c, &c->ev_knock))) return rc;
  if ((rc = c->h_knock.grow(c, std::max<uint64_t>(4, 5 * (uint64_t)n_sets)))) return rc;
  hipStream_t s = c->stream;
  GroupTimer timer(c, "k_knock");
  nemo::launch_to_host(c->h_knock.p, cs.dc.nlev + g, 4, s);
  if ((rc = wait_copied(c, c->ev_knock))) return rc;
  std::vector<knock::GraphIn> in(1);
  std::vector<uint32_t> levels(1, c->h_knock.p[0]);
  in[0] = {g, V, n_sets, knock::lds_fits(V, cs.ne(g), levels[0], c->opt.knock_lds_max)};
  const knock::Totals tot = knock::totals(in.data(), 1, cs.ko_masks);
  if (tot.limit != knock::LIMIT_OK) return ko_limit(c, "nemo_knockout_sets", tot);
  cs.ko_tab = knock::chunk_table(in.data(), 1, cs.ko_masks);
  const uint64_t n_nodes = set_off[n_sets] - set_off[0];
  if ((rc = ko_buffers(c, n_nodes, n_sets + 1, tot))) return rc;
  std::vector<uint64_t> &off = cs.ko_setoff;  // relative to the first set
  off.resize(n_sets + 1);
  for (size_t k = 0; k <= n_sets; k++) off[k] = set_off[k] - set_off[0];
  HIPCHK(c, hipMemcpyAsync(cs.d_koset.p, off.data(), (n_sets + 1) * 8, hipMemcpyHostToDevice, s));
  if (n_nodes)  // (the call ends behind a wait for the stream: the caller's array outlives the copy)
    HIPCHK(c, hipMemcpyAsync(cs.d_koleaf.p, set_nodes + set_off[0], n_nodes * 4, hipMemcpyHostToDevice, s));
  nemo::KnockArgs a{};
  a.leaf = cs.d_koleaf.p;
  a.set_off = cs.d_koset.p;
  return ko_sweep(c, a, in, levels, n_nodes, timer, 8.0 * (double)(n_sets + 1));
}

int nemo_fetch_knockout(nemo_ctx *c, nemo_knock *out, uint64_t cap, uint64_t *n_out) {
  if (!c) return NEMO_ERR_INVALID;
  if (c->node || !c->cs.ko_done)
    return fail(c, NEMO_ERR_STATE, "nemo_fetch_knockout before a knock-out call (or after a later nemo_load_corpus)");
  const uint64_t n = c->cs.ko_tab.tot.n_hyp;  // no ensure_whole: reads the last call's host rows, no graph
  if (n_out) *n_out = n;
  if (!out) return NEMO_OK;
  if (cap < n) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  if (n) memcpy(out, c->h_knock.p, n * sizeof(nemo_knock));
  return NEMO_OK;
}

int nemo_fetch_knockout_ranges(nemo_ctx *c, uint64_t *first, uint32_t *count, uint64_t cap) {
  if (!c) return NEMO_ERR_INVALID;
  if (c->node || !c->cs.ko_done)
    return fail(c, NEMO_ERR_STATE, "nemo_fetch_knockout_ranges before a knock-out call (or after a later nemo_load_corpus)");
  const knock::Table &t = c->cs.ko_tab;
  if (cap < t.first.size()) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  for (size_t i = 0; i < t.first.size(); i++) {
    if (first) first[i] = t.first[i];
    if (count) count[i] = t.count[i];
  }
  return NEMO_OK;
}

int nemo_fetch_knockout_mask(nemo_ctx *c, uint64_t hyp, uint8_t *out, uint64_t cap) {
  if (!c) return NEMO_ERR_INVALID;
  if (c->node || !c->cs.ko_done)
    return fail(c, NEMO_ERR_STATE, "nemo_fetch_knockout_mask before a knock-out call (or after a later nemo_load_corpus)");
  CorpusState &cs = c->cs;
  if (!cs.ko_masks) return fail(c, NEMO_ERR_STATE, "nemo_fetch_knockout_mask: the last knock-out call did not keep its masks (NEMO_KO_MASKS)");
  if (hyp >= cs.ko_tab.tot.n_hyp)
    return fail(c, NEMO_ERR_INVALID, "hypothesis %llu out of range (%llu hypotheses)", (unsigned long long)hyp,
                (unsigned long long)cs.ko_tab.tot.n_hyp);
  const knock::Chunk &k = cs.ko_tab.chunk[knock::chunk_of(cs.ko_tab, hyp)];
  const uint64_t V = cs.nv(k.graph);
  if (!V) return NEMO_OK;
  if (!out) return NEMO_ERR_INVALID;
  if (cap < V) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<uint64_t> w(V);  // the chunk's words; the hypothesis is one bit column of them
  HIPCHK(c, hipMemcpyAsync(w.data(), cs.d_kodead.p + k.moff, V * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint32_t bit = (uint32_t)(hyp - k.first);
  for (uint64_t v = 0; v < V; v++) out[v] = (uint8_t)((w[v] >> bit) & 1u);
  return NEMO_OK;
}

}  // extern "C"
