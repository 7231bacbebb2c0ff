// api_cuts.hip — nemo_min_cuts and its fetches (k_cuts.hip, cut_host.h; DESIGN.md §Minimal cut sets).  The rounds'
// sizes and the rows (count, scan, totals, emit, copy, stats) are knock_api.h's, shared with api_lcuts.hip.
#include "knock_api.h"

extern "C" {

// Rounds of sizes 1, 2, 3.  Round 1's words come back to the host (K / 8 bytes), which compacts the live list
// and uploads it; rounds 2 and 3 follow without a round trip; the three rounds' popcounts are scanned, the totals
// read in one blocking round trip (as nemo_diff_classes reads its hashes), the rows written and copied.
int nemo_min_cuts(nemo_ctx *c, uint32_t iteration, int cond, const uint32_t *cand, size_t n_cand, uint32_t max_size,
                  uint32_t flags) {
  if (c && c->node)
    return fail(c, NEMO_ERR_STATE, "nemo_min_cuts: single-device contexts only (a node context does not fan it out)");
  if (!c) return NEMO_ERR_INVALID;
  CorpusState &cs = c->cs;
  if (!cs.loaded) return fail(c, NEMO_ERR_STATE, "nemo_min_cuts without a loaded corpus (the last load failed?)");
  cs.cut_done = false;
  if (cond != 0 && cond != 1) return fail(c, NEMO_ERR_INVALID, "nemo_min_cuts: cond must be 0 (pre) or 1 (post)");
  if (flags) return fail(c, NEMO_ERR_INVALID, "nemo_min_cuts: unknown flags %#x", flags);
  if (max_size < 1 || max_size > CUT_MAX_SIZE) return fail(c, NEMO_ERR_INVALID, "nemo_min_cuts: max_size must be 1, 2 or 3 (%u)", max_size);
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_whole(c))) return rc;  // reads the graph's build outputs
  if ((rc = ensure_load_checked(c))) return rc;
  uint32_t r;
  if ((rc = run_index(c, iteration, &r))) return rc;
  const uint32_t g = 2 * r + (uint32_t)cond;
  const uint64_t V = cs.nv(g), E = cs.ne(g);
  if (cand) {
    size_t where = 0;
    switch (cuts::check_cands(cand, n_cand, V, &where)) {
      case cuts::CAND_RANGE:
        return fail(c, NEMO_ERR_INVALID, "nemo_min_cuts: candidate %zu is node %u, out of range (%llu nodes)", where, cand[where],
                    (unsigned long long)V);
      case cuts::CAND_DUP:
        return fail(c, NEMO_ERR_INVALID, "nemo_min_cuts: candidate %zu names node %u a second time", where, cand[where]);
      default:
        break;
    }
  }
  std::fill(cs.cut_stats, cs.cut_stats + 9, 0ull);
  cs.cut_rows = 0;
  if (cand && n_cand == 0) {  // zero hypotheses
    cs.cut_done = true;
    return NEMO_OK;
  }
  if ((rc = ensure_event(c, &c->ev_cuts))) return rc;
  if ((rc = c->h_cuts.grow(c, 8))) return rc;
  hipStream_t s = c->stream;
  GroupTimer timer(c, "k_cuts");
  if (!cs.d_cutdesc.p) {
    HIPCHK(c, hipStreamSynchronize(s));
    if ((rc = cs.d_cutdesc.grow(c, 8))) return rc;
  }
  // the graph's Kahn level count, for the tier; cand == NULL: and its sink goals, counted by k_ko_leaves
  uint32_t *desc = cs.d_cutdesc.p;  // [0] the graph | [1..2] offsets 0, K | [4..5] (sink goals, Kahn levels)
  nemo::KnockArgs ka{};
  ka.list = desc, ka.loff = desc + 1, ka.cnt = desc + 4, ka.n_list = 1;
  double bytes = 0, ops = 0;
  uint64_t K = n_cand;
  uint32_t L;
  if (!cand) {
    cs.cut_up[0] = g, cs.cut_up[1] = 0u;
    HIPCHK(c, hipMemcpyAsync(desc, cs.cut_up, 8, hipMemcpyHostToDevice, s));
    const double b_leaves = 8.0 * (double)V + 12.0;
    if ((rc = timed(c, "k_ko_leaves", b_leaves, 0, [&] { nemo::launch_ko_leaves(cs.dc, ka, false, s); }))) return rc;
    nemo::launch_to_host(c->h_cuts.p, ka.cnt, 8, s);
    if ((rc = wait_copied(c, c->ev_cuts))) return rc;
    K = c->h_cuts.p[0];
    L = c->h_cuts.p[1];
    bytes += b_leaves;
  } else {
    nemo::launch_to_host(c->h_cuts.p, cs.dc.nlev + g, 4, s);
    if ((rc = wait_copied(c, c->ev_cuts))) return rc;
    L = c->h_cuts.p[0];
  }
  cs.cut_stats[0] = K;
  if (K == 0) {  // no sink goal
    timer.done(bytes, 0);
    cs.cut_done = true;
    return NEMO_OK;
  }
  if (!cuts::round_fits(K, 1))
    return fail(c, NEMO_ERR_LIMIT, "nemo_min_cuts: %llu hypotheses of size 1 exceed 2^32 - 2: shorten the candidate list",
                (unsigned long long)K);
  // the tier and the grid: as many workgroups as are resident, at most one per chunk
  const bool lds = knock::lds_fits(V, E, L, c->opt.knock_lds_max);
  const uint32_t lds_bytes = lds ? knock::knock_lds_bytes((uint32_t)V, (uint32_t)E, L) : 0u;
  const uint64_t dw = knock::dead_words(V);
  // k_cut_glob, untuned: two workgroups per CU, fewer where their dead words (8 V bytes each) would pass CUT_DEAD_BYTES
  uint64_t resident = std::max<uint64_t>(1, std::min<uint64_t>(2ull * cs.dc.n_cu, CUT_DEAD_BYTES / (8 * std::max<uint64_t>(dw, 1))));
  if (lds) {
    for (uint32_t sz = 1; sz <= max_size; sz++) {  // the rounds' kernels: the fewest of them
      const uint32_t n = nemo::cut_lds_resident(sz, lds_bytes, cs.dc.n_cu);
      if (!n) return fail(c, NEMO_ERR_HIP, "nemo_min_cuts: no workgroup of k_cut_lds is resident at %u bytes of LDS", lds_bytes);
      resident = sz == 1 ? n : std::min<uint64_t>(resident, n);
    }
  }
  uint64_t most = K;  // an upper bound of any round's hypotheses, before the live list is known
  for (uint32_t sz = 2; sz <= max_size; sz++) most = std::max(most, std::min<uint64_t>(cuts::round_hyps(K, sz), CUT_MAX_HYPS));
  const uint64_t ck1 = cuts::chunks(K);
  {
    const uint64_t need[4] = {K, 2 * K, ck1, lds ? 1 : dw * cuts::grid(cuts::chunks(most), resident, c->opt.cut_grid)};
    if ((rc = grow_group(c, need, cs.d_cutcand, cs.d_cutlive, cs.d_cutw[0], cs.d_cutdead))) return rc;
  }
  if ((rc = c->h_cuts.grow(c, 2 * ck1 + K + 8))) return rc;
  if (cand) {
    cs.cut_cand.assign(cand, cand + K);
    HIPCHK(c, hipMemcpyAsync(cs.d_cutcand.p, cs.cut_cand.data(), K * 4, hipMemcpyHostToDevice, s));
  } else {
    cs.cut_up[2] = 0u, cs.cut_up[3] = (uint32_t)K;
    HIPCHK(c, hipMemcpyAsync(desc + 1, cs.cut_up + 2, 8, hipMemcpyHostToDevice, s));
    ka.leaf = cs.d_cutcand.p;
    const double b_leaves = 8.0 * (double)V + 12.0 + 4.0 * (double)K;
    if ((rc = timed(c, "k_ko_leaves", b_leaves, 0, [&] { nemo::launch_ko_leaves(cs.dc, ka, true, s); }))) return rc;
    bytes += b_leaves;
  }
  // one round: the byte model is the image read once per workgroup (4 E + 12 V + 4 L + 8), 8 bytes written per
  // chunk and 4 read per seed; the global tier reads the image and rewrites its 8 V dead words per chunk
  const double image = 4.0 * (double)E + 12.0 * (double)V + 4.0 * (double)L + 8.0;
  auto sweep = [&](nemo::CutArgs &a) -> int {
    if (!a.n_chunks) return NEMO_OK;
    const uint32_t grid = cuts::grid(a.n_chunks, resident, c->opt.cut_grid);
    const double seeds = 4.0 * (double)a.size * (double)a.n_hyp;
    const double b = lds ? grid * image + 8.0 * a.n_chunks + seeds : a.n_chunks * (image + 16.0 * (double)V + 8.0) + seeds;
    const double o = (double)a.n_chunks * (double)E;
    bytes += b, ops += o;
    if (lds) return timed(c, "k_cut_lds", b, o, [&] { nemo::launch_cut_lds(cs.dc, a, grid, lds_bytes, s); });
    return timed(c, "k_cut_glob", b, o, [&] { nemo::launch_cut_glob(cs.dc, a, grid, s); });
  };
  nemo::CutArgs a[3] = {};
  for (uint32_t k = 0; k < 3; k++) {
    a[k].graph = g, a[k].size = k + 1, a[k].cand = cs.d_cutcand.p, a[k].dead = cs.d_cutdead.p;
  }
  // round 1: every candidate is live
  a[0].n_hyp = (uint32_t)K, a[0].n_chunks = (uint32_t)ck1, a[0].live = nullptr, a[0].lnode = cs.d_cutcand.p;
  a[0].words = cs.d_cutw[0].p;
  if ((rc = sweep(a[0]))) return rc;
  {
    nemo::HostCopies hc;
    hc.add(c->h_cuts.p, cs.d_cutw[0].p, 8 * ck1);
    if (!cand) hc.add(c->h_cuts.p + 2 * ck1, cs.d_cutcand.p, 4 * K);
    nemo::launch_to_host_multi(hc, s);
    if ((rc = wait_copied(c, c->ev_cuts))) return rc;
  }
  if (!cand) cs.cut_cand.assign(c->h_cuts.p + 2 * ck1, c->h_cuts.p + 2 * ck1 + K);
  std::vector<uint32_t> live = cuts::live_list(reinterpret_cast<const uint64_t *>(c->h_cuts.p), K);
  const uint64_t K1 = live.size();
  CutRounds rd;
  if ((rc = cut_rounds(K, K1, max_size, [&](uint64_t k, uint32_t sz) -> int {
         if (cuts::round_fits(k, sz)) return NEMO_OK;
         return fail(c, NEMO_ERR_LIMIT, "nemo_min_cuts: the sets of %u of %llu live candidates exceed 2^32 - 2 hypotheses: shorten the candidate list",
                     sz, (unsigned long long)k);
       }, &rd)))
    return rc;
  {
    const uint64_t need[3] = {rd.ck[1], rd.ck[2], rd.scan_need};
    if ((rc = grow_group(c, need, cs.d_cutw[1], cs.d_cutw[2], cs.d_cutscan))) return rc;
  }
  if (max_size >= 2 && K1) {
    cs.cut_live.resize(2 * K1);
    for (uint64_t p = 0; p < K1; p++) {
      cs.cut_live[p] = live[p];
      cs.cut_live[K1 + p] = cs.cut_cand[live[p]];
    }
    HIPCHK(c, hipMemcpyAsync(cs.d_cutlive.p, cs.cut_live.data(), 2 * K1 * 4, hipMemcpyHostToDevice, s));
  }
  for (uint32_t k = 1; k < max_size; k++) {
    a[k].n_hyp = (uint32_t)rd.n_hyp[k], a[k].n_chunks = (uint32_t)rd.ck[k];
    a[k].live = cs.d_cutlive.p, a[k].lnode = cs.d_cutlive.p + K1;
    a[k].words = cs.d_cutw[k].p, a[k].pairs = k == 2 ? cs.d_cutw[1].p : nullptr;
    if ((rc = sweep(a[k]))) return rc;
  }
  const CutOut out = {c->h_cuts, c->ev_cuts, cs.d_cutscan, cs.d_cutrows, 4, cs.cut_stats, &cs.cut_rows, &cs.cut_done};
  return cut_rows(c, out, rd, a, max_size, timer, bytes, ops);
}

int nemo_fetch_min_cuts(nemo_ctx *c, nemo_cut *out, uint64_t cap, uint64_t *n_out) {
  if (!c) return NEMO_ERR_INVALID;
  if (c->node || !c->cs.cut_done)
    return fail(c, NEMO_ERR_STATE, "nemo_fetch_min_cuts before nemo_min_cuts (or after a later nemo_load_corpus)");
  const uint64_t n = c->cs.cut_rows;  // no ensure_whole: reads the last call's host rows, no graph
  if (n_out) *n_out = n;
  if (!out) return NEMO_OK;
  if (cap < n) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  if (n) memcpy(out, c->h_cuts.p, n * sizeof(nemo_cut));
  return NEMO_OK;
}

int nemo_fetch_min_cut_stats(nemo_ctx *c, uint64_t out[9]) {
  if (!c || !out) return NEMO_ERR_INVALID;
  if (c->node || !c->cs.cut_done)
    return fail(c, NEMO_ERR_STATE, "nemo_fetch_min_cut_stats before nemo_min_cuts (or after a later nemo_load_corpus)");
  memcpy(out, c->cs.cut_stats, sizeof c->cs.cut_stats);
  return NEMO_OK;
}

}  // extern "C"
