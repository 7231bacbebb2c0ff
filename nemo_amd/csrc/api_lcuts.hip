// api_lcuts.hip — nemo_min_label_cuts and its fetches (k_lcuts.hip, lcut_host.h; DESIGN.md §Minimal cut sets by label).
// knock_api.h holds what it shares with api_klabel.hip (the level counts, the tier split, a round's dynamic LDS), with
// api_cuts.hip (the rounds' sizes and the rows) and with api_gcuts.hip (a round's limits, launch plan and driver).
#include "knock_api.h"

extern "C" {

// The candidates are checked on the host and hashed into one table; the listed graphs go to the two tiers'
// persistent sweeps by their LDS image, as in nemo_knockout_labels.  Round 1's cut and any-hit words come back to
// the host (K / 4 bytes), which makes the live list and uploads it with its inverse; rounds 2 and 3 follow without
// a round trip; the rounds' popcounts are scanned, the totals read in one blocking round trip, the rows and their
// n_lost written and copied.
int nemo_min_label_cuts(nemo_ctx *c, const uint32_t *iters, size_t n, int cond, const uint32_t *cand_labels, size_t n_cand,
                        uint32_t max_size, uint32_t min_runs, uint32_t flags) {
  if (c && c->node)
    return fail(c, NEMO_ERR_STATE, "nemo_min_label_cuts: single-device contexts only (a node context does not fan it out)");
  if (!c) return NEMO_ERR_INVALID;
  CorpusState &cs = c->cs;
  if (!cs.loaded) return fail(c, NEMO_ERR_STATE, "nemo_min_label_cuts without a loaded corpus (the last load failed?)");
  cs.lc_done = false;  // from here on a failed call leaves no results
  if (!iters && n) return fail(c, NEMO_ERR_INVALID, "nemo_min_label_cuts: no run list for %zu list positions", n);
  if (cond != 0 && cond != 1) return fail(c, NEMO_ERR_INVALID, "nemo_min_label_cuts: cond must be 0 (pre) or 1 (post)");
  if (flags & ~NEMO_KL_SINKS) return fail(c, NEMO_ERR_INVALID, "nemo_min_label_cuts: unknown flags %#x", flags);
  if (max_size < 1 || max_size > CUT_MAX_SIZE)
    return fail(c, NEMO_ERR_INVALID, "nemo_min_label_cuts: max_size must be 1, 2 or 3 (%u)", max_size);
  uint32_t q = 0;
  if (!lcuts::min_runs(n, min_runs, &q))
    return fail(c, NEMO_ERR_INVALID, "nemo_min_label_cuts: min_runs %u exceeds the %zu list positions", min_runs, n);
  if (!cand_labels && n_cand)
    return fail(c, NEMO_ERR_INVALID, "nemo_min_label_cuts: no candidate list (there is no implicit one)");
  const uint64_t K = n_cand;
  {
    size_t where = 0;
    switch (lcuts::check_cands(cand_labels, n_cand, &where)) {
      case cuts::CAND_RANGE:
        return fail(c, NEMO_ERR_INVALID, "nemo_min_label_cuts: candidate %zu is label %u (UINT32_MAX), which is no label", where,
                    cand_labels[where]);
      case cuts::CAND_DUP:
        return fail(c, NEMO_ERR_INVALID, "nemo_min_label_cuts: candidate %zu names label %u a second time", where, cand_labels[where]);
      default:
        break;
    }
  }
  std::vector<uint32_t> &desc = cs.lc_desc;  // [n] graphs | the tiers' list positions
  desc.assign(2 * n, 0u);
  int rc;
  for (size_t i = 0; i < n; i++) {
    uint32_t r;
    if ((rc = run_index(c, iters[i], &r))) return rc;
    desc[i] = 2 * r + (uint32_t)cond;
  }
  auto limit = [&](uint64_t k, uint32_t sz) -> int { return label_round_limit(c, "nemo_min_label_cuts", "candidate list", n, k, sz); };
  if (n && K && (rc = limit(K, 1))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_whole(c))) return rc;  // may read any graph's build outputs
  if ((rc = ensure_load_checked(c))) return rc;
  std::fill(cs.lc_stats, cs.lc_stats + 9, 0ull);
  cs.lc_rows = 0;
  if (!n || !K) {  // zero hypotheses, or no list position to lose them on
    cs.lc_done = true;
    return NEMO_OK;
  }
  if ((rc = ensure_event(c, &c->ev_lcuts))) return rc;
  hipStream_t s = c->stream;
  if ((rc = ensure_nlev(c, c->h_lcuts, c->ev_lcuts))) return rc;  // (shared with nemo_knockout_labels)
  GroupTimer timer(c, "k_lcuts");
  // the tiers, the rounds' LDS and what a workgroup keeps in device memory
  const Tiers tr = split_tiers(c, desc, n);
  LabelPlan plan[3];  // K bounds every round's live positions
  uint64_t reg_need = 1;
  if ((rc = label_plans(c, "nemo_min_label_cuts", "k_lc_lds", [&](uint32_t sz, uint32_t b) { return nemo::lc_lds_resident(sz, b, cs.dc.n_cu); },
                        desc, n, tr, K, KO_LDS_STATIC, max_size, plan, &reg_need)))
    return rc;
  const uint64_t ck1 = cuts::chunks(K), slots = lcuts::table_slots(K);
  {
    const uint64_t need[10] = {K, 2 * K, K, slots, slots, 2 * (uint64_t)n, (uint64_t)n * ck1, reg_need, 2 * ck1, (uint64_t)n * ck1};
    if ((rc = grow_group(c, need, cs.d_lccand, cs.d_lcmap, cs.d_lclive, cs.d_lckey, cs.d_lcval, cs.d_lcdesc, cs.d_lchit, cs.d_lcreg,
                      cs.d_lcw[0], cs.d_lclost[0])))
      return rc;
  }
  if ((rc = c->h_lcuts.grow(c, 4 * ck1 + 8))) return rc;
  cs.lc_map.assign(2 * K, LC_NONE);
  for (uint64_t p = 0; p < K; p++) cs.lc_map[p] = (uint32_t)p;  // round 1: every candidate is live
  // (the call ends behind a wait for the stream: the caller's array outlives the copy)
  HIPCHK(c, hipMemcpyAsync(cs.d_lccand.p, cand_labels, K * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(cs.d_lcmap.p, cs.lc_map.data(), K * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(cs.d_lcdesc.p, desc.data(), 2 * n * 4, hipMemcpyHostToDevice, s));
  nemo::launch_zero(cs.d_lckey.p, 4 * slots, s);
  nemo::LcArgs a[3] = {};
  for (uint32_t k = 0; k < 3; k++) {
    a[k].cand = cs.d_lccand.p, a[k].n_cand = (uint32_t)K, a[k].key = cs.d_lckey.p, a[k].val = cs.d_lcval.p, a[k].slots = slots;
    a[k].size = k + 1, a[k].graph = cs.d_lcdesc.p, a[k].sinks = (flags & NEMO_KL_SINKS) ? 1u : 0u;
    a[k].region = cs.d_lcreg.p, a[k].n = (uint32_t)n, a[k].q = q, a[k].hit = cs.d_lchit.p;
  }
  double bytes = 0, ops = 0;
  {
    const double b = 16.0 * (double)K;  // a label read, a key and a position written, the probe
    if ((rc = timed(c, "k_lc_table", b, 0, [&] { nemo::launch_lc_table(a[0], s); }))) return rc;
    bytes += b + 4.0 * (double)slots;
  }
  // one round: the two tiers' sweeps, then the reduction (knock_api.h; its byte model with nothing more per chunk)
  auto round = [&](nemo::LcArgs &r) -> int {
    return label_round(
        c, plan[r.size - 1], tr, desc, r, cs.d_lcdesc.p, 0.0, "k_lc_lds", "k_lc_glob", [&](uint32_t grid) { nemo::launch_lc_lds(cs.dc, r, grid, s); },
        [&](uint32_t grid) { nemo::launch_lc_glob(cs.dc, r, grid, s); }, &bytes, &ops);
  };
  // round 1: every candidate is live
  a[0].lmap = cs.d_lcmap.p, a[0].k1 = (uint32_t)K, a[0].n_hyp = (uint32_t)K, a[0].n_chunks = (uint32_t)ck1;
  a[0].lost = cs.d_lclost[0].p, a[0].words = cs.d_lcw[0].p;
  if ((rc = round(a[0]))) return rc;
  nemo::launch_to_host(c->h_lcuts.p, cs.d_lcw[0].p, 16 * ck1, s);
  if ((rc = wait_copied(c, c->ev_lcuts))) return rc;
  const uint64_t *w1 = reinterpret_cast<const uint64_t *>(c->h_lcuts.p);
  cs.lc_live = lcuts::live_list(w1, w1 + ck1, K);
  const uint64_t K1 = cs.lc_live.size();
  CutRounds rd;
  if ((rc = cut_rounds(K, K1, max_size, limit, &rd))) return rc;
  {
    const uint64_t need[5] = {rd.ck[1], rd.ck[2], (uint64_t)n * rd.ck[1], (uint64_t)n * rd.ck[2], rd.scan_need};
    if ((rc = grow_group(c, need, cs.d_lcw[1], cs.d_lcw[2], cs.d_lclost[1], cs.d_lclost[2], cs.d_lcscan))) return rc;
  }
  if (max_size >= 2 && K1) {
    const std::vector<uint32_t> map = lcuts::live_map(cs.lc_live, K);
    std::copy(map.begin(), map.end(), cs.lc_map.begin() + K);
    HIPCHK(c, hipMemcpyAsync(cs.d_lcmap.p + K, cs.lc_map.data() + K, K * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(cs.d_lclive.p, cs.lc_live.data(), K1 * 4, hipMemcpyHostToDevice, s));
  }
  for (uint32_t k = 1; k < max_size; k++) {
    a[k].lmap = cs.d_lcmap.p + K, a[k].k1 = (uint32_t)K1, a[k].n_hyp = (uint32_t)rd.n_hyp[k], a[k].n_chunks = (uint32_t)rd.ck[k];
    a[k].lost = cs.d_lclost[k].p, a[k].words = cs.d_lcw[k].p, a[k].pairs = k == 2 ? cs.d_lcw[1].p : nullptr;
    if ((rc = round(a[k]))) return rc;
  }
  // the rows: k_cuts.hip's row kernels over the cut words, and behind a round's emit the recount of its rows' support
  nemo::CutArgs e[3] = {};
  for (uint32_t k = 0; k < max_size; k++) {
    e[k].size = k + 1, e[k].n_hyp = a[k].n_hyp, e[k].n_chunks = a[k].n_chunks, e[k].words = a[k].words;
    e[k].cand = cs.d_lccand.p, e[k].live = k ? cs.d_lclive.p : nullptr;
  }
  const CutOut out = {c->h_lcuts, c->ev_lcuts, cs.d_lcscan, cs.d_lcrows, 5, cs.lc_stats, &cs.lc_rows, &cs.lc_done};
  return cut_rows(c, out, rd, e, max_size, timer, bytes, ops, [&](uint32_t k, uint64_t found, uint64_t base, uint64_t rows, double *total) {
    a[k].scan = e[k].scan, a[k].n_rows = (uint32_t)found, a[k].n_lost = cs.d_lcrows.p + 4 * rows + base;
    const double b_sup = (double)found * (8.0 * (double)n + 16.0);
    *total += b_sup;
    return timed(c, "k_lc_support", b_sup, 0, [&] { nemo::launch_lc_support(a[k], s); });
  });
}

int nemo_fetch_min_label_cuts(nemo_ctx *c, nemo_label_cut *out, uint32_t *n_lost, uint64_t cap, uint64_t *n_out) {
  if (!c) return NEMO_ERR_INVALID;
  if (c->node || !c->cs.lc_done)
    return fail(c, NEMO_ERR_STATE, "nemo_fetch_min_label_cuts before nemo_min_label_cuts (or after a later nemo_load_corpus)");
  const uint64_t n = c->cs.lc_rows;  // no ensure_whole: reads the last call's host rows, no graph
  if (n_out) *n_out = n;
  if (!out) return NEMO_OK;
  if (cap < n) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  if (n) memcpy(out, c->h_lcuts.p, n * sizeof(nemo_label_cut));
  if (n && n_lost) memcpy(n_lost, c->h_lcuts.p + 4 * n, n * sizeof(uint32_t));
  return NEMO_OK;
}

int nemo_fetch_min_label_cut_stats(nemo_ctx *c, uint64_t out[9]) {
  if (!c || !out) return NEMO_ERR_INVALID;
  if (c->node || !c->cs.lc_done)
    return fail(c, NEMO_ERR_STATE, "nemo_fetch_min_label_cut_stats before nemo_min_label_cuts (or after a later nemo_load_corpus)");
  memcpy(out, c->cs.lc_stats, sizeof c->cs.lc_stats);
  return NEMO_OK;
}

}  // extern "C"
