// api_pull.hip — edge pulls: nemo_pull_edges and the fetches of its regions.
#include "ctx.h"

extern "C" {

static int pull_launch(nemo_ctx *c) {
  nemo::PullArgs &a = c->cs.pull_args;
  a.src = c->cs.d_psrc.p;
  a.dst = c->cs.d_pdst.p;
  a.cap = c->cs.d_pdst.cap;
  const uint32_t slots = c->cs.pull_dslots;
  hipStream_t s = c->stream;
  // the simplified pull reads what nemo_simplify left (graphs, flags, chains): on `aux`, behind
  // the end of the simplification only, it overlaps the protos and hand-over kernels of `stream`
  const bool on_aux = a.which == 1 && c->opt.pull_on_aux && c->ev_simp;
  if (on_aux) {
    if (!c->aux) HIPCHK(c, hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking));
    HIPCHK(c, hipStreamWaitEvent(c->aux, c->ev_simp, 0));
    s = c->aux;
  }
  double V = (double)c->cs.V, E = (double)c->cs.E;
  if (a.which < 2 && a.slot_g) V = c->cs.pl_V, E = c->cs.pl_E;  // the graphs compacted: one per class
  if (a.which == 2) {
    V = (double)slots * (double)a.mask_stride;
    E = (double)slots * (double)c->cs.ne(a.g0);
  }
  nemo::launch_zero(c->cs.d_pcur.p, sizeof(unsigned long long), s);
  // algorithmic bytes: the read side (node flags, both row pointers, columns, masks)
  uint32_t rest = c->cs.pull_rest;
  if (a.which == 2) {
    const uint64_t v0 = c->cs.nv(a.g0), e0 = c->cs.ne(a.g0);
    rest = !tier_fits(c->cs.dc.t_pull, (uint32_t)std::min<uint64_t>(v0, ~0u), (uint32_t)std::min<uint64_t>(e0, ~0u), 0);
  } else if (a.which == 3) {  // every entry has its own graph
    V = E = 0;
    rest = 0;
    for (uint32_t g : c->cs.sd_graph) {
      const uint64_t v = c->cs.nv(g), e = c->cs.ne(g);
      V += (double)v;
      E += (double)e;
      rest += !tier_fits(c->cs.dc.t_pull, (uint32_t)std::min<uint64_t>(v, ~0u), (uint32_t)std::min<uint64_t>(e, ~0u), 0);
    }
  }
  int rc = timed_on(c, s, "k_pull", 4 * E + 13 * V, E, [&] { nemo::launch_pull(c->cs.dc, a, slots, rest, s); });
  if (rc) return rc;
  nemo::HostCopies hc;
  hc.add(c->h_pull.off.p, c->cs.d_poff.p, slots * 8ull);
  hc.add(c->h_pull.cnt.p, c->cs.d_pcnt.p, slots * 4ull);
  hc.add(c->h_pull.cur.p, c->cs.d_pcur.p, sizeof(unsigned long long));
  nemo::launch_to_host_multi(hc, s);
  HIPCHK(c, hipEventRecord(c->ev_pull, s));
  if (on_aux) {
    if ((rc = ensure_event(c, &c->ev_auxpull))) return rc;
    HIPCHK(c, hipEventRecord(c->ev_auxpull, s));
    c->cs.pull_aux_pending = true;
  }
  c->cs.pull_synced = false;
  return NEMO_OK;
}

static int pull_grow(nemo_ctx *c, uint64_t total) {
  if (total <= c->cs.d_pdst.cap) return NEMO_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->cs.d_psrc.release(c), c->cs.d_pdst.release(c);
  if (int rc = c->cs.d_psrc.grow(c, total)) return rc;
  return c->cs.d_pdst.grow(c, total);
}

// Wait for the last pull's slot table; re-run it once if its regions overran the capacity.
static int pull_sync(nemo_ctx *c) {
  if (c->cs.pull_synced) return NEMO_OK;
  HIPCHK(c, hipEventSynchronize(c->ev_pull));
  const uint64_t total = *c->h_pull.cur.p;
  if (total > c->cs.d_pdst.cap) {
    int rc = pull_grow(c, total);
    if (!rc) rc = pull_launch(c);
    if (rc) return rc;
    HIPCHK(c, hipEventSynchronize(c->ev_pull));
  }
  c->cs.pull_hint[c->cs.pull_which] = total;
  if (c->cs.pull_expand) {  // shared regions: slot e takes its computed slot's (map[e] <= e)
    for (uint32_t e = c->cs.pull_slots; e-- > 0;) {
      const uint32_t u = c->cs.pull_expand[e];
      c->h_pull.off.p[e] = c->h_pull.off.p[u];
      c->h_pull.cnt.p[e] = c->h_pull.cnt.p[u];
    }
    c->cs.pull_expand = nullptr;
  }
  c->cs.pull_synced = true;
  return NEMO_OK;
}

// The slot list of a raw / simplified pull over the duplicate-graph classes (gdedup::pull_plan), made at the
// first such pull after a load or a change of the pull's LDS tier and uploaded once.  The graphs past that
// tier keep slots of their own: k_pull and k_mwp_* take duplicates like any graph, as the global tiers of the
// other kernels do.  The tier is judged by the sizes, as everywhere on the host: a class inside the caps but
// deeper than the tier's level cap shares a slot here and k_pull takes that one slot.  The big graphs' slots
// follow the list on the device (PullArgs::big_slot: the chunk table keeps a row per big graph).
// *use: some graph shares a slot (else the launches are the ones without classes).
static int pull_plan(nemo_ctx *c, bool *use) {
  CorpusState &s = c->cs;
  const Tier &t = s.dc.t_pull;
  if (!s.pl_ok || t.v != s.pl_tier.v || t.e != s.pl_tier.e || t.l != s.pl_tier.l || t.bytes != s.pl_tier.bytes) {
    std::vector<uint8_t> apart(s.G);
    for (uint32_t g = 0; g < s.G; g++)
      apart[g] = !t.bytes || !tier_fits(t, (uint32_t)std::min<uint64_t>(s.nv(g), ~0u), (uint32_t)std::min<uint64_t>(s.ne(g), ~0u), 0);
    s.pl = gdedup::pull_plan(s.gd_rep, apart);
    s.pl_V = s.pl_E = 0;
    for (uint32_t g : s.pl.list) s.pl_V += (double)s.nv(g), s.pl_E += (double)s.ne(g);
    for (uint32_t g = 0; g < s.G; g++)
      if (s.pl.map[g] > g) return fail(c, NEMO_ERR_STATE, "pull plan: graph %u's slot lies after it", g);
    // a pull still reading the old list finishes first (a tier change is an option change: rare)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->aux) HIPCHK(c, hipStreamSynchronize(c->aux));
    std::vector<uint32_t> up(s.pl.list);  // the list, then at G the big graphs' slots
    up.resize(s.G);
    for (uint32_t g : s.big_host) up.push_back(s.pl.map[g]);
    if (int rc = s.d_pl_list.grow(c, (uint64_t)s.G + s.big_host.size())) return rc;
    HIPCHK(c, hipMemcpyAsync(s.d_pl_list.p, up.data(), 4 * up.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s.pl_tier = t;
    s.pl_ok = true;
  }
  *use = s.pl.list.size() < s.G;
  return NEMO_OK;
}

int nemo_pull_edges(nemo_ctx *c, int which) {
  DISPATCH(node_pull_edges(c, which));
  if (!c || which < 0 || which > 3) return NEMO_ERR_INVALID;
  if (!c->cs.loaded) return fail(c, NEMO_ERR_STATE, "no corpus loaded");
  if (which == 1 && !c->cs.simplified) return fail(c, NEMO_ERR_STATE, "simplified pull before nemo_simplify");
  if (which == 3 && !c->cs.sd_done)
    return fail(c, NEMO_ERR_STATE, "symmetric diff pull (which 3) before nemo_diffprov_symmetric");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = ensure_load_checked(c);
  if (rc) return rc;
  const uint32_t slots = which == 2 ? c->cs.n_entries : which == 3 ? c->cs.n_sentries : c->cs.G;
  // the previous pull's slot table may still be in flight into the pinned tables: wait for it
  // only when they are about to be reallocated (a pull queued behind another on the same
  // stream overwrites the device tables in order; the host reads them in pull_sync after the
  // last pull's event)
  const bool grow_slots = (uint64_t)slots + 1 > c->cs.d_pcnt.cap || !c->cs.d_poff.p;
  if (!c->cs.pull_synced && (grow_slots || (uint64_t)slots + 1 > c->h_pull.cap()))
    HIPCHK(c, hipEventSynchronize(c->ev_pull));
  c->cs.pull_synced = true;
  if (which == 2 && (rc = join_aux(c))) return rc;  // the D masks
  // diff entries sharing a label source have one D mask, hence one graph: it is
  // compacted once and their slots share its region (pull_sync expands the table)
  const bool share = which == 2 && c->cs.n_uniq < c->cs.n_entries;
  // graphs of identical content have one raw and one simplified edge list (node indices are graph-local):
  // one graph per class is compacted and every graph of the class shares its region (pull_plan)
  bool classes = which < 2 && c->cs.dc.dd_list && c->opt.pull_dedup;
  if (classes && (rc = pull_plan(c, &classes))) return rc;
  // which 0 / 1 over the classes compacts the listed graphs only, and those are representatives while the
  // slices are stale (every graph inside the tier: device_load); which 2 reads run 0's post graph
  if ((rc = which == 2 ? ensure_run0(c) : which < 2 && classes ? NEMO_OK : ensure_whole(c))) return rc;
  const uint32_t dslots = share ? c->cs.n_uniq : classes ? (uint32_t)c->cs.pl.list.size() : slots;
  if ((rc = ensure_event(c, &c->ev_pull))) return rc;
  if ((rc = c->cs.d_pcur.grow(c, 1))) return rc;
  if (grow_slots) {
    c->cs.d_pcnt.release(c), c->cs.d_poff.release(c);
    if ((rc = c->cs.d_pcnt.grow(c, (uint64_t)slots + 1)) || (rc = c->cs.d_poff.grow(c, (uint64_t)slots + 1))) return rc;
  }
  if ((rc = c->h_pull.grow(c, (uint64_t)slots + 1))) return rc;
  c->cs.pull_which = which;
  c->cs.pull_slots = slots;
  c->cs.pull_dslots = dslots;
  if (share) c->cs.pull_map = c->cs.dmap;
  else c->cs.pull_map.clear();
  c->cs.pull_expand = share ? c->cs.pull_map.data() : classes ? c->cs.pl.map.data() : nullptr;
  if (slots == 0) return NEMO_OK;
  nemo::PullArgs a{};
  a.which = (uint32_t)which;
  a.g0 = c->cs.run0 >= 0 ? c->cs.g0() : 0;
  uint64_t cap;
  if (which == 2) {
    a.mask = c->cs.d_dmask.p;
    a.mask_stride = c->cs.V0();
    a.mask_row = share ? c->cs.d_dsrc.p + 2 * c->cs.n_entries : nullptr;  // diffprov's representative entries
    cap = (uint64_t)dslots * c->cs.E0();  // D is an induced subgraph of g0
  } else if (which == 3) {
    // slot = entry, graph = the entry's failed post graph, liveness = its S mask (ragged)
    a.slot_g = c->cs.d_sdgraph.p;
    a.mask = c->cs.d_sdmask.p;
    a.mask_off = c->cs.d_sdoff.p;
    cap = 0;  // S is an induced subgraph of the entry's graph
    for (uint32_t g : c->cs.sd_graph) cap += c->cs.ne(g);
  } else {
    if (classes) a.slot_g = c->cs.d_pl_list.p, a.big_slot = c->cs.d_pl_list.p + c->cs.G;
    const uint64_t E = classes ? (uint64_t)c->cs.pl_E : c->cs.E;  // of the graphs compacted
    // which 0: every edge; which 1: kept edges (<= E) + collapsed edges; a pull past the estimate re-runs on fetch
    cap = which == 0 ? E : std::max<uint64_t>(2 * E + 1024, c->cs.pull_hint[1] + c->cs.pull_hint[1] / 4);
  }
  a.cnt = c->cs.d_pcnt.p;
  a.off = c->cs.d_poff.p;
  a.cursor = c->cs.d_pcur.p;
  // big graphs' chunk table (k_diff.hip MWP_CH = 4096 nodes or chains per chunk)
  a.ccnt = nullptr;
  a.maxck = 0;
  uint32_t rows = which == 2 ? (c->cs.V0() >= NEMO_CSR_BIG ? dslots : 0u) : c->cs.dc.n_big;
  if (which == 3) {  // a chunk-table row per entry as soon as one entry's graph is big
    rows = 0;
    for (uint32_t g : c->cs.sd_graph)
      if (c->cs.nv(g) >= NEMO_CSR_BIG) rows = dslots;
  }
  if (rows) {
    a.maxck = (uint32_t)(2 * ((c->cs.bigVmax + 4095) / 4096));
    const size_t need = (size_t)rows * a.maxck;
    if (need > c->cs.d_pck.cap) {
      HIPCHK(c, hipStreamSynchronize(c->stream));  // a previous pull may still use the chunk table
      if ((rc = c->cs.d_pck.grow(c, need))) return rc;
    }
    a.ccnt = c->cs.d_pck.p;
  }
  c->cs.pull_args = a;
  if ((rc = pull_grow(c, std::max<uint64_t>(cap, 1)))) return rc;
  return pull_launch(c);
}

uint64_t nemo_pulled_count(nemo_ctx *c, uint32_t slot) {
  DISPATCH(node_pulled_count(c, slot));
  if (!c || c->cs.pull_which < 0 || slot >= c->cs.pull_slots) return 0;
  if (pull_sync(c)) return 0;  // no ensure_whole: reads the pull's slot table, no graph
  return c->h_pull.cnt.p[slot];
}

int nemo_fetch_pulled(nemo_ctx *c, uint32_t slot, uint32_t *src, uint32_t *dst, uint64_t cap, uint64_t *n_out) {
  DISPATCH(node_fetch_pulled(c, slot, src, dst, cap, n_out));
  if (!c) return NEMO_ERR_INVALID;
  if (c->cs.pull_which < 0) return fail(c, NEMO_ERR_STATE, "nothing pulled");
  if (slot >= c->cs.pull_slots) return fail(c, NEMO_ERR_INVALID, "slot %u out of range", slot);
  HIPCHK(c, hipSetDevice(c->device));
  // no ensure_whole: reads the pulled regions, no graph
  int rc = pull_sync(c);
  if (rc) return rc;
  const uint64_t a = c->h_pull.off.p[slot], n = c->h_pull.cnt.p[slot];
  if (n_out) *n_out = n;
  if (!src && !dst) return NEMO_OK;
  if (cap < n) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  if (n) {
    if (src) HIPCHK(c, hipMemcpyAsync(src, c->cs.d_psrc.p + a, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (dst) HIPCHK(c, hipMemcpyAsync(dst, c->cs.d_pdst.p + a, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return NEMO_OK;
}

int nemo_fetch_pulled_all(nemo_ctx *c, uint64_t *off, uint32_t *cnt, uint32_t *src, uint32_t *dst, uint64_t cap,
                          uint64_t *n_used) {
  DISPATCH(node_fetch_pulled_all(c, off, cnt, src, dst, cap, n_used));
  if (!c) return NEMO_ERR_INVALID;
  if (c->cs.pull_which < 0) return fail(c, NEMO_ERR_STATE, "nothing pulled");
  HIPCHK(c, hipSetDevice(c->device));
  // no ensure_whole: reads the pulled regions, no graph
  int rc = pull_sync(c);
  if (rc) return rc;
  const uint64_t used = c->cs.pull_slots ? *c->h_pull.cur.p : 0;
  if (n_used) *n_used = used;
  if (off && c->cs.pull_slots) memcpy(off, c->h_pull.off.p, c->cs.pull_slots * 8ull);
  if (cnt && c->cs.pull_slots) memcpy(cnt, c->h_pull.cnt.p, c->cs.pull_slots * 4ull);
  if (!src && !dst) return NEMO_OK;
  if (cap < used) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  if (used) {
    if (src) HIPCHK(c, hipMemcpyAsync(src, c->cs.d_psrc.p, used * 4, hipMemcpyDeviceToHost, c->stream));
    if (dst) HIPCHK(c, hipMemcpyAsync(dst, c->cs.d_pdst.p, used * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return NEMO_OK;
}

}  // extern "C"
