// api_klabel.hip — nemo_knockout_labels and its fetches (k_klabel.hip, klabel_host.h; DESIGN.md §Knock-out by label).
// The level counts, the tier split and the launch's dynamic LDS are knock_api.h's, shared with api_lcuts.hip.
#include "knock_api.h"

extern "C" {

// The label sets are checked and sized on the host (klabel_host.h), uploaded once and hashed into one table per
// chunk of 64 sets (k_kl_tables); the listed graphs go to the two tiers' persistent sweeps by their LDS image
// (the Kahn level counts are read once per load); k_kl_count sums the bit columns; one copy brings the words and
// the counts to pinned memory.
int nemo_knockout_labels(nemo_ctx *c, const uint32_t *iters, size_t n, int cond, const uint64_t *set_off,
                         const uint32_t *set_labels, size_t n_sets, uint32_t flags) {
  if (c && c->node)
    return fail(c, NEMO_ERR_STATE, "nemo_knockout_labels: single-device contexts only (a node context does not fan it out)");
  if (!c || (!iters && n) || (!set_off && n_sets)) return NEMO_ERR_INVALID;
  CorpusState &cs = c->cs;
  if (!cs.loaded) return fail(c, NEMO_ERR_STATE, "nemo_knockout_labels without a loaded corpus (the last load failed?)");
  cs.kl_done = false;
  if (cond != 0 && cond != 1) return fail(c, NEMO_ERR_INVALID, "nemo_knockout_labels: cond must be 0 (pre) or 1 (post)");
  if (flags & ~NEMO_KL_SINKS) return fail(c, NEMO_ERR_INVALID, "nemo_knockout_labels: unknown flags %#x", flags);
  if (!klabel::sets_fit(n_sets))  // before set_off is read
    return fail(c, NEMO_ERR_LIMIT, "nemo_knockout_labels: %zu sets exceed 2^32 - 1 in one call: tile the call", n_sets);
  uint64_t where = 0;
  switch (klabel::check_offsets(set_off, n_sets, &where)) {  // before any label is read
    case klabel::SET_NONMONOTONE:
      return fail(c, NEMO_ERR_INVALID, "nemo_knockout_labels: set_off decreases at set %llu", (unsigned long long)where);
    case klabel::SET_LIMIT:
      return fail(c, NEMO_ERR_LIMIT, "nemo_knockout_labels: the sets name more than 2^32 - 1 labels: tile the call");
    default:
      break;
  }
  const uint64_t n_labels = n_sets ? set_off[n_sets] - set_off[0] : 0;
  if (n_labels && !set_labels) return NEMO_ERR_INVALID;
  if (klabel::check_sets(set_off, set_labels, n_sets, &where) == klabel::SET_LABEL)
    return fail(c, NEMO_ERR_INVALID, "nemo_knockout_labels: the label at position %llu is UINT32_MAX, which is no label",
                (unsigned long long)where);
  std::vector<uint32_t> &desc = cs.kl_desc;  // [n] graphs | the tiers' list positions
  desc.assign(2 * n, 0u);
  int rc;
  for (size_t i = 0; i < n; i++) {
    uint32_t r;
    if ((rc = run_index(c, iters[i], &r))) return rc;
    desc[i] = 2 * r + (uint32_t)cond;
  }
  if (!klabel::words_fit(n, n_sets))
    return fail(c, NEMO_ERR_LIMIT, "nemo_knockout_labels: %zu list positions x %llu chunks of 64 sets exceed 2^28 words: tile the call", n,
                (unsigned long long)klabel::chunks(n_sets));
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_whole(c))) return rc;  // may read any graph's build outputs
  if ((rc = ensure_load_checked(c))) return rc;
  const uint64_t ck = klabel::chunks(n_sets), words = (uint64_t)n * ck;
  cs.kl_n = n, cs.kl_sets = n_sets, cs.kl_chunks = ck;
  if (!n || !n_sets) {  // zero words
    cs.kl_done = true;
    return NEMO_OK;
  }
  if ((rc = ensure_event(c, &c->ev_klabel))) return rc;
  hipStream_t s = c->stream;
  if ((rc = ensure_nlev(c, c->h_klabel, c->ev_klabel))) return rc;
  GroupTimer timer(c, "k_klabel");
  // the tiers, the launch's LDS and what a workgroup keeps in device memory
  const Tiers tr = split_tiers(c, desc, n);
  const uint32_t n_lds = tr.n_lds, n_glob = tr.n_glob;
  const uint64_t glob_v = tr.glob_v;
  uint32_t lds_total = 0, res_lds = 1;
  uint64_t spill = 0;
  if (n_lds) {
    const bool list = c->opt.kl_hitlist;  // no hit list: nothing to keep behind the image
    if ((rc = ko_lds_total(c, "nemo_knockout_labels", "k_kl_lds", [&](uint32_t b) { return nemo::kl_lds_resident(b, cs.dc.n_cu, list); },
                           tr.image, list ? UINT32_MAX : 0, KO_LDS_STATIC, &lds_total, &res_lds)))
      return rc;
    for (size_t k = 0; k < n_lds; k++) {
      const uint32_t g = desc[desc[n + k]];
      const uint64_t head = (lds_total - tier_image(c, g)) / 8u;
      spill = std::max<uint64_t>(spill, cs.nv(g) > head ? cs.nv(g) - head : 0);
    }
  }
  const uint32_t cap = c->opt.kl_grid;
  const uint64_t rw_lds = klabel::region_words(0, spill), rw_glob = klabel::region_words(knock::dead_words(glob_v), glob_v);
  uint64_t r_lds = klabel::region_grid(res_lds, rw_lds), r_glob = klabel::region_grid(2ull * cs.dc.n_cu, rw_glob);
  if (cap) r_lds = std::min<uint64_t>(r_lds, cap), r_glob = std::min<uint64_t>(r_glob, cap);
  const klabel::Split sp_lds = klabel::split(n_lds, ck, r_lds), sp_glob = klabel::split(n_glob, ck, r_glob);
  const uint32_t grid_lds = klabel::grid(sp_lds.items, r_lds, cap), grid_glob = klabel::grid(sp_glob.items, r_glob, cap);
  // the tables and the buffers
  std::vector<uint64_t> &off = cs.kl_setoff;  // relative to the first set
  off.resize(n_sets + 1);
  for (size_t k = 0; k <= n_sets; k++) off[k] = set_off[k] - set_off[0];
  cs.kl_taboff = klabel::table_offsets(off.data(), n_sets);
  const uint64_t slots = cs.kl_taboff[ck + 1], mslots = cs.kl_taboff[ck];
  const uint64_t out_words = 2 * words + 64 * ck;  // the word pairs, then 2 x 64 u32 counts per chunk
  {
    const uint64_t need[8] = {n_sets + 1, std::max<uint64_t>(n_labels, 1), ck + 2, slots, mslots, 2 * (uint64_t)n, out_words,
                              std::max<uint64_t>(1, std::max<uint64_t>(n_lds ? grid_lds * rw_lds : 0ull, n_glob ? grid_glob * rw_glob : 0ull))};
    if ((rc = grow_group(c, need, cs.d_klset, cs.d_kllab, cs.d_kltoff, cs.d_klkey, cs.d_klmask, cs.d_kldesc, cs.d_klout, cs.d_klreg)))
      return rc;
  }
  if ((rc = c->h_klabel.grow(c, out_words))) return rc;
  HIPCHK(c, hipMemcpyAsync(cs.d_klset.p, off.data(), (n_sets + 1) * 8, hipMemcpyHostToDevice, s));
  if (n_labels)  // (the call ends behind a wait for the stream: the caller's array outlives the copy)
    HIPCHK(c, hipMemcpyAsync(cs.d_kllab.p, set_labels + set_off[0], n_labels * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(cs.d_kltoff.p, cs.kl_taboff.data(), (ck + 2) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(cs.d_kldesc.p, desc.data(), 2 * n * 4, hipMemcpyHostToDevice, s));
  nemo::launch_zero(cs.d_klkey.p, 4 * slots, s);
  nemo::launch_zero(cs.d_klmask.p, 8 * mslots, s);
  nemo::KlArgs a{};
  a.set_off = cs.d_klset.p, a.labels = cs.d_kllab.p, a.n_sets = (uint32_t)n_sets, a.n_chunks = (uint32_t)ck;
  a.tab_off = cs.d_kltoff.p, a.key = cs.d_klkey.p, a.mask = cs.d_klmask.p;
  a.graph = cs.d_kldesc.p, a.sinks = (flags & NEMO_KL_SINKS) ? 1u : 0u;
  a.no_list = c->opt.kl_hitlist ? 0u : 1u;
  a.region = cs.d_klreg.p, a.out = cs.d_klout.p, a.n = (uint32_t)n;
  a.cnt = reinterpret_cast<uint32_t *>(cs.d_klout.p + 2 * words);
  // the byte model: the tables take every label once (4 read, 2 x 12 of table traffic) and their zeroes; a work
  // item reads its graph's image (4 E + 12 V + 4 L + 8) and 4 V labels; a chunk writes 16 bytes and probes 12
  // bytes per hit, at most min(V, labels) of them (the host does not know the hit count); ops = E child words per
  // chunk; the global tier adds 16 V per chunk for its dead words in device memory (8 V written, 8 V read);
  // without the hit list (option kl_hitlist 0) a chunk reads 4 V labels and probes V times
  const double b_tab = 28.0 * (double)n_labels + 8.0 * (double)(n_sets + 1) + 4.0 * (double)slots + 8.0 * (double)mslots;
  if ((rc = timed(c, "k_kl_tables", b_tab, 0, [&] { nemo::launch_kl_tables(a, s); }))) return rc;
  double bytes = b_tab, ops = 0;
  for (int tier = 0; tier < 2; tier++) {
    const uint32_t nt = tier ? n_glob : n_lds;
    if (!nt) continue;
    const klabel::Split &sp = tier ? sp_glob : sp_lds;
    double b = 0, o = 0;
    for (uint32_t k = 0; k < nt; k++) {
      const uint32_t g = desc[desc[n + (tier ? n_lds : 0) + k]];
      const double V = (double)cs.nv(g), E = (double)cs.ne(g), L = (double)cs.kl_nlev[g];
      b += sp.parts * (4.0 * E + 12.0 * V + 4.0 * L + 8.0 + 4.0 * V) + (double)ck * (a.no_list && !tier ? 16.0 + 16.0 * V : 16.0 + 12.0 * std::min(V, (double)n_labels)) +
           (tier ? (double)ck * 16.0 * V : 0.0);
      o += (double)ck * E;
    }
    a.pos = cs.d_kldesc.p + n + (tier ? n_lds : 0);
    a.n_tier = nt, a.parts = sp.parts;
    a.lds_total = tier ? 0u : lds_total;
    a.region_words = tier ? rw_glob : rw_lds;
    a.dead_words = tier ? knock::dead_words(glob_v) : 0;
    if (tier) rc = timed(c, "k_kl_glob", b, o, [&] { nemo::launch_kl_glob(cs.dc, a, grid_glob, s); });
    else rc = timed(c, "k_kl_lds", b, o, [&] { nemo::launch_kl_lds(cs.dc, a, grid_lds, s); });
    if (rc) return rc;
    bytes += b, ops += o;
  }
  const double b_cnt = 16.0 * (double)words + 512.0 * (double)ck;
  if ((rc = timed(c, "k_kl_count", b_cnt, 0, [&] { nemo::launch_kl_count(a, s); }))) return rc;
  timer.done(bytes + b_cnt, ops);
  nemo::launch_to_host(c->h_klabel.p, cs.d_klout.p, 8 * out_words, s);
  if ((rc = wait_copied(c, c->ev_klabel))) return rc;
  cs.kl_done = true;
  return NEMO_OK;
}

int nemo_fetch_knockout_labels(nemo_ctx *c, uint64_t *lost, uint64_t *hit, uint64_t cap_words) {
  if (!c) return NEMO_ERR_INVALID;
  if (c->node || !c->cs.kl_done)
    return fail(c, NEMO_ERR_STATE, "nemo_fetch_knockout_labels before nemo_knockout_labels (or after a later nemo_load_corpus)");
  const CorpusState &cs = c->cs;  // no ensure_whole: reads the last call's host words, no graph
  const uint64_t words = cs.kl_n && cs.kl_sets ? cs.kl_n * cs.kl_chunks : 0;
  if (cap_words < words) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  for (uint64_t k = 0; k < words; k++) {
    if (lost) lost[k] = c->h_klabel.p[2 * k];
    if (hit) hit[k] = c->h_klabel.p[2 * k + 1];
  }
  return NEMO_OK;
}

int nemo_fetch_knockout_label_counts(nemo_ctx *c, uint32_t *n_lost, uint32_t *n_hit, uint64_t cap) {
  if (!c) return NEMO_ERR_INVALID;
  if (c->node || !c->cs.kl_done)
    return fail(c, NEMO_ERR_STATE, "nemo_fetch_knockout_label_counts before nemo_knockout_labels (or after a later nemo_load_corpus)");
  const CorpusState &cs = c->cs;
  if (cap < cs.kl_sets) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  const bool none = !cs.kl_n || !cs.kl_sets;  // no list position: nothing was counted
  const uint32_t *cnt = none ? nullptr : reinterpret_cast<const uint32_t *>(c->h_klabel.p + 2 * cs.kl_n * cs.kl_chunks);
  for (uint64_t k = 0; k < cs.kl_sets; k++) {
    if (n_lost) n_lost[k] = none ? 0u : cnt[k];
    if (n_hit) n_hit[k] = none ? 0u : cnt[64 * cs.kl_chunks + k];
  }
  return NEMO_OK;
}

}  // extern "C"
