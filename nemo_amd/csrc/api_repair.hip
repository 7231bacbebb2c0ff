// api_repair.hip — nemo_min_repair_sets, nemo_min_repairs and their fetches (k_repair.hip, repair_host.h; DESIGN.md
// §Minimal repair sets).  The rounds' sizes and the rows (count, scan, totals, emit, copy, stats) are knock_api.h's,
// shared with api_cuts.hip; the ranks, the live list and the grid are cut_host.h's.
#include "knock_api.h"

namespace {

// What the two forms share once the graph is known: the entry checks are done, nothing is queued yet.
struct RepairCall {
  const char *who;
  uint32_t g;         // 2r + cond
  uint32_t max_size;
};

int repair_begin(nemo_ctx *c, const char *who, uint32_t max_size, uint32_t flags) {
  if (c && c->node) return fail(c, NEMO_ERR_STATE, "%s: single-device contexts only (a node context does not fan it out)", who);
  if (!c) return NEMO_ERR_INVALID;
  if (!c->cs.loaded) return fail(c, NEMO_ERR_STATE, "%s without a loaded corpus (the last load failed?)", who);
  c->cs.rp_done = false;
  if (flags) return fail(c, NEMO_ERR_INVALID, "%s: unknown flags %#x", who, flags);
  if (max_size < 1 || max_size > CUT_MAX_SIZE) return fail(c, NEMO_ERR_INVALID, "%s: max_size must be 1, 2 or 3 (%u)", who, max_size);
  return NEMO_OK;
}

// a call that ends before the search: its status, |A| and no rows
int repair_end(nemo_ctx *c, uint32_t status, uint64_t n_absent) {
  CorpusState &cs = c->cs;
  std::fill(cs.rp_stats, cs.rp_stats + 11, 0ull);
  cs.rp_stats[0] = status, cs.rp_stats[1] = n_absent;
  cs.rp_rows = 0;
  cs.rp_done = true;
  return NEMO_OK;
}

// The search over graph rc.g with the bitmap in d_rpbits and the K candidates in d_rpcand (both queued on the
// stream), L Kahn levels and n_absent absent nodes.  from_dev: cs.rp_cand is not known yet (the pair form) and
// comes back with rounds 0 and 1's words.  Rounds 0 and 1 run back to back and their words come back in one copy;
// the host decides the status and the live list; rounds 2 and 3 follow without a round trip; the rows are cut_rows'.
int repair_search(nemo_ctx *c, const RepairCall &rc_, uint64_t K, uint32_t L, uint64_t n_absent, bool from_dev, GroupTimer &timer,
                  double bytes) {
  CorpusState &cs = c->cs;
  const char *who = rc_.who;
  const uint32_t g = rc_.g, max_size = rc_.max_size;
  const uint64_t V = cs.nv(g), E = cs.ne(g);
  hipStream_t s = c->stream;
  int rc;
  double ops = 0;
  if (!cuts::round_fits(K, 1))
    return fail(c, NEMO_ERR_LIMIT, "%s: %llu hypotheses of size 1 exceed 2^32 - 2: shorten the candidate list", who, (unsigned long long)K);
  // the tier and the grid: as many workgroups as are resident, at most one per chunk
  const bool lds = repair::lds_fits(V, E, L, c->opt.knock_lds_max);
  const uint32_t lds_bytes = lds ? repair::repair_lds_bytes((uint32_t)V, (uint32_t)E, L) : 0u;
  const uint64_t dw = knock::dead_words(V), bw = repair::bitmap_words(V);
  // k_repair_glob, untuned: two workgroups per CU, fewer where their dead words (8 V bytes each) would pass CUT_DEAD_BYTES
  uint64_t resident = std::max<uint64_t>(1, std::min<uint64_t>(2ull * cs.dc.n_cu, CUT_DEAD_BYTES / (8 * std::max<uint64_t>(dw, 1))));
  if (lds) {
    for (uint32_t sz = 0; sz <= max_size; sz++) {  // the rounds' kernels: the fewest of them
      const uint32_t n = nemo::repair_lds_resident(sz, lds_bytes, cs.dc.n_cu);
      if (!n) return fail(c, NEMO_ERR_HIP, "%s: no workgroup of k_repair_lds is resident at %u bytes of LDS", who, lds_bytes);
      resident = sz == 0 ? n : std::min<uint64_t>(resident, n);
    }
  }
  uint64_t most = std::max<uint64_t>(K, 1);  // an upper bound of any round's hypotheses, before the live list is known
  for (uint32_t sz = 2; sz <= max_size; sz++) most = std::max(most, std::min<uint64_t>(cuts::round_hyps(K, sz), CUT_MAX_HYPS));
  const uint64_t ck1 = cuts::chunks(K);
  {
    const uint64_t need[3] = {2 * K, ck1 + 1, lds ? 1 : dw * cuts::grid(cuts::chunks(most), resident, c->opt.cut_grid)};
    if ((rc = grow_group(c, need, cs.d_rplive, cs.d_rpw[0], cs.d_rpdead))) return rc;
  }
  if ((rc = c->h_repair.grow(c, 2 * (ck1 + 1) + K + 8))) return rc;
  // one round: nemo_min_cuts' byte model plus the bitmap (8 bw bytes), read once per workgroup on the LDS tier and
  // once per chunk on the global tier
  const double image = 4.0 * (double)E + 12.0 * (double)V + 4.0 * (double)L + 8.0 + 8.0 * (double)bw;
  auto sweep = [&](const nemo::CutArgs &a) -> int {
    if (!a.n_chunks) return NEMO_OK;
    nemo::RepairArgs ra{a, cs.d_rpbits.p, (uint32_t)K};
    const uint32_t grid = cuts::grid(a.n_chunks, resident, c->opt.cut_grid);
    const double seeds = a.size ? 4.0 * (double)a.size * (double)a.n_hyp : 4.0 * (double)K;
    const double b = lds ? grid * image + 8.0 * a.n_chunks + seeds : a.n_chunks * (image + 16.0 * (double)V + 8.0) + seeds;
    const double o = (double)a.n_chunks * (double)E;
    bytes += b, ops += o;
    if (lds) return timed(c, "k_repair_lds", b, o, [&] { nemo::launch_repair_lds(cs.dc, ra, grid, lds_bytes, s); });
    return timed(c, "k_repair_glob", b, o, [&] { nemo::launch_repair_glob(cs.dc, ra, grid, s); });
  };
  nemo::CutArgs a[3] = {};
  for (uint32_t k = 0; k < 3; k++) {
    a[k].graph = g, a[k].size = k + 1, a[k].cand = cs.d_rpcand.p, a[k].dead = cs.d_rpdead.p;
  }
  // round 0: one chunk, its word behind round 1's
  nemo::CutArgs a0 = a[0];
  a0.size = 0, a0.n_hyp = 2, a0.n_chunks = 1, a0.words = cs.d_rpw[0].p + ck1;
  if ((rc = sweep(a0))) return rc;
  // round 1: every candidate is live
  a[0].n_hyp = (uint32_t)K, a[0].n_chunks = (uint32_t)ck1, a[0].live = nullptr, a[0].lnode = cs.d_rpcand.p;
  a[0].words = cs.d_rpw[0].p;
  if ((rc = sweep(a[0]))) return rc;
  {
    nemo::HostCopies hc;
    hc.add(c->h_repair.p, cs.d_rpw[0].p, 8 * (ck1 + 1));
    if (from_dev) hc.add(c->h_repair.p + 2 * (ck1 + 1), cs.d_rpcand.p, 4 * K);
    nemo::launch_to_host_multi(hc, s);
    if ((rc = wait_copied(c, c->ev_repair))) return rc;
  }
  if (from_dev) cs.rp_cand.assign(c->h_repair.p + 2 * (ck1 + 1), c->h_repair.p + 2 * (ck1 + 1) + K);
  const uint64_t *w1 = reinterpret_cast<const uint64_t *>(c->h_repair.p);
  const uint32_t status = repair::status(w1[ck1]);
  if (status != REPAIR_SEARCHED) {  // round 1 was wasted
    timer.done(bytes, ops);
    return repair_end(c, status, n_absent);
  }
  std::vector<uint32_t> live = cuts::live_list(w1, K);  // the candidates that are no repair alone
  const uint64_t K1 = live.size();
  CutRounds rd;
  if ((rc = cut_rounds(K, K1, max_size, [&](uint64_t k, uint32_t sz) -> int {
         if (cuts::round_fits(k, sz)) return NEMO_OK;
         return fail(c, NEMO_ERR_LIMIT, "%s: the sets of %u of %llu live candidates exceed 2^32 - 2 hypotheses: shorten the candidate list", who,
                     sz, (unsigned long long)k);
       }, &rd)))
    return rc;
  {
    const uint64_t need[3] = {rd.ck[1], rd.ck[2], rd.scan_need};
    if ((rc = grow_group(c, need, cs.d_rpw[1], cs.d_rpw[2], cs.d_rpscan))) return rc;
  }
  if (max_size >= 2 && K1) {
    cs.rp_live.resize(2 * K1);
    for (uint64_t p = 0; p < K1; p++) {
      cs.rp_live[p] = live[p];
      cs.rp_live[K1 + p] = cs.rp_cand[live[p]];
    }
    HIPCHK(c, hipMemcpyAsync(cs.d_rplive.p, cs.rp_live.data(), 2 * K1 * 4, hipMemcpyHostToDevice, s));
  }
  for (uint32_t k = 1; k < max_size; k++) {
    a[k].n_hyp = (uint32_t)rd.n_hyp[k], a[k].n_chunks = (uint32_t)rd.ck[k];
    a[k].live = cs.d_rplive.p, a[k].lnode = cs.d_rplive.p + K1;
    a[k].words = cs.d_rpw[k].p, a[k].pairs = k == 2 ? cs.d_rpw[1].p : nullptr;
    if ((rc = sweep(a[k]))) return rc;
  }
  std::fill(cs.rp_stats, cs.rp_stats + 11, 0ull);
  cs.rp_stats[0] = REPAIR_SEARCHED, cs.rp_stats[1] = n_absent;
  const CutOut out = {c->h_repair, c->ev_repair, cs.d_rpscan, cs.d_rprows, 4, cs.rp_stats + 2, &cs.rp_rows, &cs.rp_done};
  return cut_rows(c, out, rd, a, max_size, timer, bytes, ops);
}

}  // namespace

extern "C" {

int nemo_min_repair_sets(nemo_ctx *c, uint32_t iteration, int cond, const uint32_t *absent, size_t n_absent, const uint32_t *cand,
                         size_t n_cand, uint32_t max_size, uint32_t flags) {
  const char *who = "nemo_min_repair_sets";
  int rc;
  if ((rc = repair_begin(c, who, max_size, flags))) return rc;
  CorpusState &cs = c->cs;
  if (cond != 0 && cond != 1) return fail(c, NEMO_ERR_INVALID, "%s: cond must be 0 (pre) or 1 (post)", who);
  if ((!absent && n_absent) || (cand && !absent && n_cand)) return fail(c, NEMO_ERR_INVALID, "%s: a null absent list", who);
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_whole(c))) return rc;  // reads the graph's build outputs
  if ((rc = ensure_load_checked(c))) return rc;
  uint32_t r;
  if ((rc = run_index(c, iteration, &r))) return rc;
  const uint32_t g = 2 * r + (uint32_t)cond;
  const uint64_t V = cs.nv(g);
  {
    size_t where = 0;
    switch (repair::check_lists(absent, n_absent, cand, n_cand, V, &where)) {
      case repair::ABSENT_RANGE:
        return fail(c, NEMO_ERR_INVALID, "%s: absent node %zu is node %u, out of range (%llu nodes)", who, where, absent[where],
                    (unsigned long long)V);
      case repair::ABSENT_DUP:
        return fail(c, NEMO_ERR_INVALID, "%s: absent node %zu names node %u a second time", who, where, absent[where]);
      case repair::CAND_DUP:
        return fail(c, NEMO_ERR_INVALID, "%s: candidate %zu names node %u a second time", who, where, cand[where]);
      case repair::CAND_NOT_ABSENT:
        return fail(c, NEMO_ERR_INVALID, "%s: candidate %zu is node %u, which is not in the absent list", who, where, cand[where]);
      default:
        break;
    }
  }
  const uint64_t K = cand ? n_cand : n_absent;
  cs.rp_cand.assign(cand ? cand : absent, (cand ? cand : absent) + K);
  if (n_absent == 0) return repair_end(c, REPAIR_HOLDS, 0);  // nothing is lost
  if ((rc = ensure_event(c, &c->ev_repair))) return rc;
  if ((rc = c->h_repair.grow(c, 8))) return rc;
  hipStream_t s = c->stream;
  GroupTimer timer(c, "k_repair");
  {
    const uint64_t need[2] = {repair::bitmap_words(V), std::max<uint64_t>(K, 1)};
    if ((rc = grow_group(c, need, cs.d_rpbits, cs.d_rpcand))) return rc;
  }
  cs.rp_bits = repair::bitmap(absent, n_absent, V);
  HIPCHK(c, hipMemcpyAsync(cs.d_rpbits.p, cs.rp_bits.data(), 8 * cs.rp_bits.size(), hipMemcpyHostToDevice, s));
  if (K) HIPCHK(c, hipMemcpyAsync(cs.d_rpcand.p, cs.rp_cand.data(), 4 * K, hipMemcpyHostToDevice, s));
  nemo::launch_to_host(c->h_repair.p, cs.dc.nlev + g, 4, s);  // the graph's Kahn level count, for the tier
  if ((rc = wait_copied(c, c->ev_repair))) return rc;
  const uint32_t L = c->h_repair.p[0];
  return repair_search(c, {who, g, max_size}, K, L, n_absent, false, timer, 0.0);
}

// The pair form: A = cand = the sink goals of base's post graph whose label is no goal label of other's post graph,
// made on the device.  The other run's table is the load's for run 0, else k_lab_hash's, as nemo_diffprov_pairs'.
int nemo_min_repairs(nemo_ctx *c, uint32_t base_iter, uint32_t other_iter, uint32_t max_size, uint32_t flags) {
  const char *who = "nemo_min_repairs";
  int rc;
  if ((rc = repair_begin(c, who, max_size, flags))) return rc;
  CorpusState &cs = c->cs;
  if (!cs.marked) return fail(c, NEMO_ERR_STATE, "%s before nemo_mark_holds", who);
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_whole(c))) return rc;  // reads both graphs
  if ((rc = ensure_load_checked(c))) return rc;
  uint32_t rb, ro;
  if ((rc = run_index(c, base_iter, &rb)) || (rc = run_index(c, other_iter, &ro))) return rc;
  const uint32_t g = 2 * rb + 1, go = 2 * ro + 1;
  const uint64_t V = cs.nv(g);
  cs.rp_cand.clear();
  if (V == 0) return repair_end(c, REPAIR_HOLDS, 0);
  const pairs::Plan plan = pairs::plan(&go, 1, cs.node_off.data(), cs.run0 >= 0 ? (int64_t)cs.g0() : -1);
  if (!plan.ok) return fail(c, NEMO_ERR_LIMIT, "%s: a label table would exceed 2^32 slots", who);
  const bool shared = plan.entry_tab[0] == PAIRS_SHARED;
  if ((rc = ensure_event(c, &c->ev_repair))) return rc;
  if ((rc = c->h_repair.grow(c, 8))) return rc;
  hipStream_t s = c->stream;
  GroupTimer timer(c, "k_repair");
  if (!cs.d_rpcnt.p || (!shared && (!cs.d_rptab.p || plan.words > cs.d_rphreg.cap || !cs.d_rphreg.p))) {
    HIPCHK(c, hipStreamSynchronize(s));  // an earlier call may still use them
    if ((rc = cs.d_rpcnt.grow(c, 2))) return rc;
    if (!shared && ((rc = cs.d_rptab.grow(c, 1)) || (rc = cs.d_rphreg.grow(c, plan.words)))) return rc;
  }
  {
    const uint64_t need[2] = {repair::bitmap_words(V), V};
    if ((rc = grow_group(c, need, cs.d_rpbits, cs.d_rpcand))) return rc;
  }
  double bytes = 0;
  cs.rp_tab = shared ? nemo::LabTab{cs.d_r0hkey, cs.r0hmask, go} : nemo::LabTab{cs.d_rphreg.p, plan.tab_mask[0], go};
  if (!shared) {
    HIPCHK(c, hipMemcpyAsync(cs.d_rptab.p, &cs.rp_tab, sizeof(nemo::LabTab), hipMemcpyHostToDevice, s));
    const uint32_t lds_max = c->opt.pair_hash_lds_max;
    const uint32_t lds_slots = plan.tab_mask[0] < lds_max ? plan.tab_mask[0] + 1u : 0u;
    const double b = 8.0 * (double)plan.nodes + 4.0 * (double)plan.words;
    if ((rc = timed(c, "k_lab_hash", b, 0, [&] { nemo::launch_lab_hash(cs.dc, cs.d_rptab.p, 1, lds_max, lds_slots, s); }))) return rc;
    bytes += b;
  }
  {
    // node word, label and two row pointers of every node, a probe per sink goal, the bitmap and the list written
    const double b = 20.0 * (double)V + (double)V / 8.0 + 8.0;
    if ((rc = timed(c, "k_repair_absent", b, 0, [&] {
           nemo::launch_repair_absent(cs.dc, g, cs.rp_tab.key, cs.rp_tab.mask, cs.d_rpbits.p, cs.d_rpcand.p, cs.d_rpcnt.p, s);
         })))
      return rc;
    bytes += b;
  }
  nemo::launch_to_host(c->h_repair.p, cs.d_rpcnt.p, 8, s);  // the count beside the Kahn level count
  if ((rc = wait_copied(c, c->ev_repair))) return rc;
  const uint64_t K = c->h_repair.p[0];
  const uint32_t L = c->h_repair.p[1];
  if (K == 0) {  // every sink goal's label is a goal label of the other run
    timer.done(bytes, 0);
    return repair_end(c, REPAIR_HOLDS, 0);
  }
  return repair_search(c, {who, g, max_size}, K, L, K, true, timer, bytes);
}

int nemo_fetch_min_repairs(nemo_ctx *c, nemo_repair *out, uint64_t cap, uint64_t *n_out) {
  if (!c) return NEMO_ERR_INVALID;
  if (c->node || !c->cs.rp_done)
    return fail(c, NEMO_ERR_STATE, "nemo_fetch_min_repairs before nemo_min_repair_sets / nemo_min_repairs (or after a later nemo_load_corpus)");
  const uint64_t n = c->cs.rp_rows;  // no ensure_whole: reads the last call's host rows, no graph
  if (n_out) *n_out = n;
  if (!out) return NEMO_OK;
  if (cap < n) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  if (n) memcpy(out, c->h_repair.p, n * sizeof(nemo_repair));
  return NEMO_OK;
}

int nemo_fetch_min_repair_stats(nemo_ctx *c, uint64_t out[11]) {
  if (!c || !out) return NEMO_ERR_INVALID;
  if (c->node || !c->cs.rp_done)
    return fail(c, NEMO_ERR_STATE, "nemo_fetch_min_repair_stats before nemo_min_repair_sets / nemo_min_repairs (or after a later nemo_load_corpus)");
  memcpy(out, c->cs.rp_stats, sizeof c->cs.rp_stats);
  return NEMO_OK;
}

int nemo_fetch_min_repair_cands(nemo_ctx *c, uint32_t *out, uint64_t cap, uint64_t *n_out) {
  if (!c) return NEMO_ERR_INVALID;
  if (c->node || !c->cs.rp_done)
    return fail(c, NEMO_ERR_STATE, "nemo_fetch_min_repair_cands before nemo_min_repair_sets / nemo_min_repairs (or after a later nemo_load_corpus)");
  const uint64_t n = c->cs.rp_cand.size();
  if (n_out) *n_out = n;
  if (!out) return NEMO_OK;
  if (cap < n) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  if (n) memcpy(out, c->cs.rp_cand.data(), n * 4);
  return NEMO_OK;
}

}  // extern "C"
