// api_gcuts.hip — nemo_min_group_cuts and its fetches (k_gcuts.hip, gcut_host.h; DESIGN.md §Minimal cut sets over
// fault events).  knock_api.h holds what it shares with api_klabel.hip and api_lcuts.hip (the level counts, the tier
// split, a round's dynamic LDS), with api_cuts.hip and api_lcuts.hip (the rounds' sizes and the rows) and with
// api_lcuts.hip alone (a round's limits, launch plan and driver); the reduction and the recount of a row's support
// are k_lcuts.hip's kernels on the round's LcArgs.
#include "gcut_host.h"
#include "knock_api.h"

// What a workgroup of k_gc_lds takes of a CU's LDS beside its dynamic part: the kernel's static LDS (1,840 bytes
// in round 3 by the compiler's report, profiles/r19_gc_kernel_resources.txt), rounded up to whole allocation
// granules with one to spare (KO_LDS_STATIC's rule).
#define GC_LDS_STATIC 2560

extern "C" {

// The groups are checked on the host, which also counts their distinct labels D (the bound of a workgroup's hit
// list); the offsets (as u32 from the first group's) and the labels are uploaded, k_gc_table / k_gc_rows turn the
// labels into rows of one table.  From there on the call is nemo_min_label_cuts': the two tiers' persistent sweeps,
// round 1's cut and any-hit words to the host (K / 4 bytes), which makes the live list and uploads it; rounds 2 and
// 3 without a round trip; the popcounts scanned, the totals read in one blocking round trip, the rows and their
// n_lost written and copied.
int nemo_min_group_cuts(nemo_ctx *c, const uint32_t *iters, size_t n, int cond, const uint64_t *group_off, const uint32_t *group_labels,
                        size_t n_groups, uint32_t max_size, uint32_t min_runs, uint32_t flags) {
  if (c && c->node)
    return fail(c, NEMO_ERR_STATE, "nemo_min_group_cuts: single-device contexts only (a node context does not fan it out)");
  if (!c) return NEMO_ERR_INVALID;
  CorpusState &cs = c->cs;
  if (!cs.loaded) return fail(c, NEMO_ERR_STATE, "nemo_min_group_cuts without a loaded corpus (the last load failed?)");
  cs.gc_done = false;  // from here on a failed call leaves no results
  if (!iters && n) return fail(c, NEMO_ERR_INVALID, "nemo_min_group_cuts: no run list for %zu list positions", n);
  if (cond != 0 && cond != 1) return fail(c, NEMO_ERR_INVALID, "nemo_min_group_cuts: cond must be 0 (pre) or 1 (post)");
  if (flags & ~NEMO_KL_SINKS) return fail(c, NEMO_ERR_INVALID, "nemo_min_group_cuts: unknown flags %#x", flags);
  if (max_size < 1 || max_size > CUT_MAX_SIZE)
    return fail(c, NEMO_ERR_INVALID, "nemo_min_group_cuts: max_size must be 1, 2 or 3 (%u)", max_size);
  uint32_t q = 0;
  if (!lcuts::min_runs(n, min_runs, &q))
    return fail(c, NEMO_ERR_INVALID, "nemo_min_group_cuts: min_runs %u exceeds the %zu list positions", min_runs, n);
  if (!group_off && n_groups)
    return fail(c, NEMO_ERR_INVALID, "nemo_min_group_cuts: no group_off for %zu groups (there is no implicit event list)", n_groups);
  const uint64_t K = n_groups;
  {
    uint64_t group = 0, where = 0;
    switch (klabel::check_offsets(group_off, n_groups, &group)) {  // before any label is read
      case klabel::SET_NONMONOTONE:
        return fail(c, NEMO_ERR_INVALID, "nemo_min_group_cuts: group_off decreases at group %llu", (unsigned long long)group);
      case klabel::SET_LIMIT:
        return fail(c, NEMO_ERR_LIMIT, "nemo_min_group_cuts: the groups name more than 2^32 - 1 labels in all: shorten the group list");
      default:
        break;
    }
    for (size_t k = 0; k < n_groups; k++)  // ... and this: from the offsets alone
      if (group_off[k + 1] - group_off[k] > GC_MAX_GROUP)
        return fail(c, NEMO_ERR_LIMIT, "nemo_min_group_cuts: group %zu names %llu labels, more than 2^24: split the group", k,
                    (unsigned long long)(group_off[k + 1] - group_off[k]));
    if (!group_labels && gcuts::named(group_off, n_groups))
      return fail(c, NEMO_ERR_INVALID, "nemo_min_group_cuts: no group_labels for the %llu labels the groups name",
                  (unsigned long long)gcuts::named(group_off, n_groups));
    if (gcuts::check_groups(group_off, group_labels, n_groups, &group, &where) == gcuts::GROUP_LABEL)
      return fail(c, NEMO_ERR_INVALID, "nemo_min_group_cuts: group %llu names label UINT32_MAX, which is no label, at position %llu",
                  (unsigned long long)group, (unsigned long long)where);
  }
  std::vector<uint32_t> &desc = cs.gc_desc;  // [n] graphs | the tiers' list positions
  desc.assign(2 * n, 0u);
  int rc;
  for (size_t i = 0; i < n; i++) {
    uint32_t r;
    if ((rc = run_index(c, iters[i], &r))) return rc;
    desc[i] = 2 * r + (uint32_t)cond;
  }
  auto limit = [&](uint64_t k, uint32_t sz) -> int { return label_round_limit(c, "nemo_min_group_cuts", "group list", n, k, sz); };
  if (n && K && (rc = limit(K, 1))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_whole(c))) return rc;  // may read any graph's build outputs
  if ((rc = ensure_load_checked(c))) return rc;
  std::fill(cs.gc_stats, cs.gc_stats + 9, 0ull);
  cs.gc_rows = 0;
  if (!n || !K) {  // zero hypotheses, or no list position to lose them on
    cs.gc_done = true;
    return NEMO_OK;
  }
  if ((rc = ensure_event(c, &c->ev_gcuts))) return rc;
  hipStream_t s = c->stream;
  if ((rc = ensure_nlev(c, c->h_gcuts, c->ev_gcuts))) return rc;  // (shared with nemo_knockout_labels)
  GroupTimer timer(c, "k_gcuts");
  const uint64_t T = gcuts::named(group_off, n_groups), D = gcuts::distinct_labels(group_off, group_labels, n_groups);
  // the tiers, the rounds' LDS and what a workgroup keeps in device memory: D + 1 + V entries of hit list
  const Tiers tr = split_tiers(c, desc, n);
  if (!gcuts::list_fits(D, std::max(tr.lds_v, tr.glob_v)))
    return fail(c, NEMO_ERR_LIMIT,
                "nemo_min_group_cuts: %llu distinct labels and a graph of %llu nodes exceed 2^32 - 1 hit-list entries: shorten the group list",
                (unsigned long long)D, (unsigned long long)std::max(tr.lds_v, tr.glob_v));
  LabelPlan plan[3];
  uint64_t reg_need = 1;
  if ((rc = label_plans(c, "nemo_min_group_cuts", "k_gc_lds", [&](uint32_t sz, uint32_t b) { return nemo::gc_lds_resident(sz, b, cs.dc.n_cu); },
                        desc, n, tr, D, GC_LDS_STATIC, max_size, plan, &reg_need)))
    return rc;
  const uint64_t ck1 = cuts::chunks(K), slots = gcuts::table_slots(D);
  {
    const uint64_t need[11] = {K + 1, std::max<uint64_t>(T, 1), K, K, slots + 1, slots, 2 * (uint64_t)n, (uint64_t)n * ck1, reg_need, 2 * ck1, (uint64_t)n * ck1};
    if ((rc = grow_group(c, need, cs.d_gcoff, cs.d_gcgrow, cs.d_gcident, cs.d_gclive, cs.d_gckey, cs.d_gcval, cs.d_gcdesc, cs.d_gchit,
                      cs.d_gcreg, cs.d_gcw[0], cs.d_gclost[0])))
      return rc;
  }
  if ((rc = c->h_gcuts.grow(c, 4 * ck1 + 8))) return rc;
  cs.gc_off = gcuts::offsets32(group_off, n_groups);
  cs.gc_ident.resize(K);
  for (uint64_t p = 0; p < K; p++) cs.gc_ident[p] = (uint32_t)p;
  // (the call ends behind a wait for the stream: the caller's array outlives the copy)
  HIPCHK(c, hipMemcpyAsync(cs.d_gcoff.p, cs.gc_off.data(), (K + 1) * 4, hipMemcpyHostToDevice, s));
  if (T) HIPCHK(c, hipMemcpyAsync(cs.d_gcgrow.p, group_labels + group_off[0], T * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(cs.d_gcident.p, cs.gc_ident.data(), K * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(cs.d_gcdesc.p, desc.data(), 2 * n * 4, hipMemcpyHostToDevice, s));
  nemo::launch_zero(cs.d_gckey.p, 4 * (slots + 1), s);  // the keys and, behind them, the rows handed out
  nemo::GcArgs a[3] = {};
  for (uint32_t k = 0; k < 3; k++) {
    nemo::LcArgs &r = a[k].r;
    r.key = cs.d_gckey.p, r.val = cs.d_gcval.p, r.slots = slots;
    r.size = k + 1, r.graph = cs.d_gcdesc.p, r.sinks = (flags & NEMO_KL_SINKS) ? 1u : 0u;
    r.region = cs.d_gcreg.p, r.n = (uint32_t)n, r.q = q, r.hit = cs.d_gchit.p;
    a[k].goff = cs.d_gcoff.p, a[k].grow = cs.d_gcgrow.p, a[k].n_named = (uint32_t)T, a[k].n_dist = (uint32_t)D;
    a[k].n_rows = cs.d_gckey.p + slots;
  }
  double bytes = 0, ops = 0;
  {
    const double b = 16.0 * (double)T;  // a label read, a key and a row written, the probe; per kernel
    if ((rc = timed(c, "k_gc_table", b, 0, [&] { nemo::launch_gc_table(a[0], s); }))) return rc;
    if ((rc = timed(c, "k_gc_rows", b, 0, [&] { nemo::launch_gc_rows(a[0], s); }))) return rc;
    bytes += 2.0 * b + 4.0 * (double)slots;
  }
  // One round: the two tiers' sweeps, then the reduction (knock_api.h).  Its byte model, and per chunk the groups of
  // the 64 sets: two offsets and on average T / K rows, 4 bytes each, per set and group.
  const double per_set = 8.0 + 4.0 * (double)T / (double)K;
  auto round = [&](nemo::GcArgs &ga) -> int {
    return label_round(
        c, plan[ga.r.size - 1], tr, desc, ga.r, cs.d_gcdesc.p, 64.0 * ga.r.size * per_set, "k_gc_lds", "k_gc_glob",
        [&](uint32_t grid) { nemo::launch_gc_lds(cs.dc, ga, grid, s); }, [&](uint32_t grid) { nemo::launch_gc_glob(cs.dc, ga, grid, s); }, &bytes, &ops);
  };
  // round 1: every candidate is live
  a[0].live = nullptr, a[0].r.n_hyp = (uint32_t)K, a[0].r.n_chunks = (uint32_t)ck1;
  a[0].r.lost = cs.d_gclost[0].p, a[0].r.words = cs.d_gcw[0].p;
  if ((rc = round(a[0]))) return rc;
  nemo::launch_to_host(c->h_gcuts.p, cs.d_gcw[0].p, 16 * ck1, s);
  if ((rc = wait_copied(c, c->ev_gcuts))) return rc;
  const uint64_t *w1 = reinterpret_cast<const uint64_t *>(c->h_gcuts.p);
  cs.gc_live = lcuts::live_list(w1, w1 + ck1, K);
  const uint64_t K1 = cs.gc_live.size();
  CutRounds rd;
  if ((rc = cut_rounds(K, K1, max_size, limit, &rd))) return rc;
  {
    const uint64_t need[5] = {rd.ck[1], rd.ck[2], (uint64_t)n * rd.ck[1], (uint64_t)n * rd.ck[2], rd.scan_need};
    if ((rc = grow_group(c, need, cs.d_gcw[1], cs.d_gcw[2], cs.d_gclost[1], cs.d_gclost[2], cs.d_gcscan))) return rc;
  }
  if (max_size >= 2 && K1) HIPCHK(c, hipMemcpyAsync(cs.d_gclive.p, cs.gc_live.data(), K1 * 4, hipMemcpyHostToDevice, s));
  for (uint32_t k = 1; k < max_size; k++) {
    a[k].live = cs.d_gclive.p, a[k].r.n_hyp = (uint32_t)rd.n_hyp[k], a[k].r.n_chunks = (uint32_t)rd.ck[k];
    a[k].r.lost = cs.d_gclost[k].p, a[k].r.words = cs.d_gcw[k].p, a[k].r.pairs = k == 2 ? cs.d_gcw[1].p : nullptr;
    if ((rc = round(a[k]))) return rc;
  }
  // the rows: k_cuts.hip's row kernels over the cut words (a row's entries are candidate positions: `cand` is the
  // identity), and behind a round's emit k_lc_support's recount of its rows' support
  nemo::CutArgs e[3] = {};
  for (uint32_t k = 0; k < max_size; k++) {
    e[k].size = k + 1, e[k].n_hyp = a[k].r.n_hyp, e[k].n_chunks = a[k].r.n_chunks, e[k].words = a[k].r.words;
    e[k].cand = cs.d_gcident.p, e[k].live = k ? cs.d_gclive.p : nullptr;
  }
  const CutOut out = {c->h_gcuts, c->ev_gcuts, cs.d_gcscan, cs.d_gcrows, 5, cs.gc_stats, &cs.gc_rows, &cs.gc_done};
  return cut_rows(c, out, rd, e, max_size, timer, bytes, ops, [&](uint32_t k, uint64_t found, uint64_t base, uint64_t rows, double *total) {
    nemo::LcArgs &r = a[k].r;
    r.scan = e[k].scan, r.n_rows = (uint32_t)found, r.n_lost = cs.d_gcrows.p + 4 * rows + base;
    const double b_sup = (double)found * (8.0 * (double)n + 16.0);
    *total += b_sup;
    return timed(c, "k_lc_support", b_sup, 0, [&] { nemo::launch_lc_support(r, s); });
  });
}

int nemo_fetch_min_group_cuts(nemo_ctx *c, nemo_group_cut *out, uint32_t *n_lost, uint64_t cap, uint64_t *n_out) {
  if (!c) return NEMO_ERR_INVALID;
  if (c->node || !c->cs.gc_done)
    return fail(c, NEMO_ERR_STATE, "nemo_fetch_min_group_cuts before nemo_min_group_cuts (or after a later nemo_load_corpus)");
  const uint64_t n = c->cs.gc_rows;  // no ensure_whole: reads the last call's host rows, no graph
  if (n_out) *n_out = n;
  if (!out) return NEMO_OK;
  if (cap < n) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  if (n) memcpy(out, c->h_gcuts.p, n * sizeof(nemo_group_cut));
  if (n && n_lost) memcpy(n_lost, c->h_gcuts.p + 4 * n, n * sizeof(uint32_t));
  return NEMO_OK;
}

int nemo_fetch_min_group_cut_stats(nemo_ctx *c, uint64_t out[9]) {
  if (!c || !out) return NEMO_ERR_INVALID;
  if (c->node || !c->cs.gc_done)
    return fail(c, NEMO_ERR_STATE, "nemo_fetch_min_group_cut_stats before nemo_min_group_cuts (or after a later nemo_load_corpus)");
  memcpy(out, c->cs.gc_stats, sizeof c->cs.gc_stats);
  return NEMO_OK;
}

}  // extern "C"
