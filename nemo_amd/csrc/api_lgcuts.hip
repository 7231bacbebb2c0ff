// api_lgcuts.hip — nemo_lineage_group_cuts and its fetches (k_lgcuts.hip, lgc_host.h; DESIGN.md §Lineage cut search
// over fault events).  The checks of the groups are nemo_min_group_cuts' (gcut_host.h), the label -> row table its
// kernels', the tier rule and image the witness calls' (wit_host.h), the keys, the tables, the filter and the level
// loop nemo_lineage_cuts' (lin_host.h, k_lineage.hip, lin_api.h's lin_levels).  The host drives the levels: per level it
// queues the evaluation on either tier, the cross-run count and the filter, reads one block of three counters from
// pinned memory, and decides whether the level runs again behind a grown emission buffer.
#include "gcut_host.h"
#include "knock_api.h"
#include "lin_api.h"

// What a workgroup of k_lgc_lds takes of a CU's LDS beside its dynamic part: the kernel's static LDS (the chunk's keys,
// a scan of 64 lengths and offsets, four words), rounded up generously as k_lin_lds's.  A value too small cannot cost a
// resident workgroup: ko_lds_total's second query refuses the larger size then.
#define LGC_LDS_STATIC 4096

namespace {

int lgc_empty(CorpusState &cs) {  // zero rows, every stat 0
  cs.lg_done = true;
  return NEMO_OK;
}

}  // namespace

extern "C" {

int nemo_lineage_group_cuts(nemo_ctx *c, const uint32_t *iters, size_t n, int cond, const uint64_t *group_off, const uint32_t *group_labels,
                            size_t n_groups, uint32_t max_size, uint32_t min_runs, uint32_t flags) {
  static const char *const who = "nemo_lineage_group_cuts";
  if (c && c->node)
    return fail(c, NEMO_ERR_STATE, "nemo_lineage_group_cuts: single-device contexts only (a node context does not fan it out)");
  if (!c) return NEMO_ERR_INVALID;
  CorpusState &cs = c->cs;
  if (!cs.loaded) return fail(c, NEMO_ERR_STATE, "nemo_lineage_group_cuts without a loaded corpus (the last load failed?)");
  cs.lg_done = false;  // from here on a failed call leaves no results
  if (!iters && n) return fail(c, NEMO_ERR_INVALID, "nemo_lineage_group_cuts: no run list for %zu list positions", n);
  if (cond != 0 && cond != 1) return fail(c, NEMO_ERR_INVALID, "nemo_lineage_group_cuts: cond must be 0 (pre) or 1 (post)");
  if (flags & ~NEMO_KL_SINKS) return fail(c, NEMO_ERR_INVALID, "nemo_lineage_group_cuts: unknown flags %#x", flags);
  if (!lgc::size_ok(max_size)) return fail(c, NEMO_ERR_INVALID, "nemo_lineage_group_cuts: max_size must be 1..8 (%u)", max_size);
  uint32_t q = 0;
  if (!lcuts::min_runs(n, min_runs, &q))
    return fail(c, NEMO_ERR_INVALID, "nemo_lineage_group_cuts: min_runs %u exceeds the %zu list positions", min_runs, n);
  if (!group_off && n_groups)
    return fail(c, NEMO_ERR_INVALID, "nemo_lineage_group_cuts: no group_off for %zu groups (there is no implicit event list)", n_groups);
  if (!lgc::groups_fit(n_groups))  // before the offsets are read
    return fail(c, NEMO_ERR_LIMIT, "nemo_lineage_group_cuts: %zu groups exceed 65535 (a set is eight u16 candidate positions): shorten the group list",
                n_groups);
  const uint64_t K = n_groups;
  {
    uint64_t group = 0, where = 0;
    switch (klabel::check_offsets(group_off, n_groups, &group)) {  // before any label is read
      case klabel::SET_NONMONOTONE:
        return fail(c, NEMO_ERR_INVALID, "nemo_lineage_group_cuts: group_off decreases at group %llu", (unsigned long long)group);
      case klabel::SET_LIMIT:
        return fail(c, NEMO_ERR_LIMIT, "nemo_lineage_group_cuts: the groups name more than 2^32 - 1 labels in all: shorten the group list");
      default:
        break;
    }
    for (size_t k = 0; k < n_groups; k++)  // ... and this: from the offsets alone
      if (group_off[k + 1] - group_off[k] > GC_MAX_GROUP)
        return fail(c, NEMO_ERR_LIMIT, "nemo_lineage_group_cuts: group %zu names %llu labels, more than 2^24: split the group", k,
                    (unsigned long long)(group_off[k + 1] - group_off[k]));
    if (!group_labels && gcuts::named(group_off, n_groups))
      return fail(c, NEMO_ERR_INVALID, "nemo_lineage_group_cuts: no group_labels for the %llu labels the groups name",
                  (unsigned long long)gcuts::named(group_off, n_groups));
    if (gcuts::check_groups(group_off, group_labels, n_groups, &group, &where) == gcuts::GROUP_LABEL)
      return fail(c, NEMO_ERR_INVALID, "nemo_lineage_group_cuts: group %llu names label UINT32_MAX, which is no label, at position %llu",
                  (unsigned long long)group, (unsigned long long)where);
  }
  int rc;
  auto level_limit = [&](uint64_t n_front, uint32_t d) -> int {
    switch (lgc::level_check(n, n_front)) {
      case lgc::LEVEL_FRONT:
        return fail(c, NEMO_ERR_LIMIT, "nemo_lineage_group_cuts: a frontier of %llu sets of size %u exceeds 2^32 - 2: shorten the group list",
                    (unsigned long long)n_front, d);
      case lgc::LEVEL_WORDS:
        return fail(c, NEMO_ERR_LIMIT,
                    "nemo_lineage_group_cuts: %zu list positions x %llu chunks of 64 sets of size %u exceed 2^28 words: shorten the group list or the run list",
                    n, (unsigned long long)lin::chunks(n_front), d);
      default:
        return NEMO_OK;
    }
  };
  if (n && K && (rc = level_limit(1, 0))) return rc;  // level 0, from the sizes alone: before the run list is read
  std::vector<uint32_t> &desc = cs.lg_desc;  // [n] graphs | the tiers' list positions
  desc.assign(2 * n, 0u);
  for (size_t i = 0; i < n; i++) {
    uint32_t r;
    if ((rc = run_index(c, iters[i], &r))) return rc;
    desc[i] = 2 * r + (uint32_t)cond;
  }
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_whole(c))) return rc;  // may read any graph's build outputs
  if ((rc = ensure_load_checked(c))) return rc;
  std::fill(cs.lg_stats, cs.lg_stats + 18, 0ull);
  cs.lg_rows.clear();
  cs.lg_nlost.clear();
  if (!n || !K) return lgc_empty(cs);  // no candidate, or no list position to lose a set on
  if ((rc = ensure_event(c, &c->ev_lgc))) return rc;
  hipStream_t s = c->stream;
  if ((rc = ensure_nlev(c, c->h_lgc, c->ev_lgc))) return rc;
  {
    bool any = false;
    for (size_t i = 0; i < n && !any; i++) any = cs.nv(desc[i]) != 0 && cs.kl_nlev[desc[i]] != 0;
    if (!any) return lgc_empty(cs);  // no root anywhere: nothing is ever lost
  }
  if ((rc = c->h_lgc.grow(c, 8))) return rc;
  GroupTimer timer(c, "k_lgcuts");
  const uint64_t T = gcuts::named(group_off, n_groups), D = gcuts::distinct_labels(group_off, group_labels, n_groups);
  // the tiers (the witness calls' image and option), the launch's LDS and what a workgroup keeps in device memory
  const uint32_t lds_max = c->opt.wit_lds_max;
  auto fits = [&](uint32_t g) { return wit::lds_fits(cs.nv(g), cs.ne(g), cs.kl_nlev[g], lds_max); };
  auto image = [&](uint32_t g) { return wit::wit_lds_bytes((uint32_t)cs.nv(g), (uint32_t)cs.ne(g), cs.kl_nlev[g]); };
  const Tiers tr = split_tiers_by(c, desc, n, fits, image);
  if (!gcuts::list_fits(D, std::max(tr.lds_v, tr.glob_v)))
    return fail(c, NEMO_ERR_LIMIT,
                "nemo_lineage_group_cuts: %llu distinct labels and a graph of %llu nodes exceed 2^32 - 1 hit-list entries: shorten the group list",
                (unsigned long long)D, (unsigned long long)std::max(tr.lds_v, tr.glob_v));
  uint32_t lds_total = 0, res_lds = 1;
  uint64_t rw_lds = 0;
  if (tr.n_lds) {
    if ((rc = ko_lds_total(c, who, "k_lgc_lds", [&](uint32_t b) { return nemo::lgc_lds_resident(b, cs.dc.n_cu); }, tr.image,
                           lgc::tail_want(D, tr.lds_v), LGC_LDS_STATIC, &lds_total, &res_lds)))
      return rc;
    for (size_t k = 0; k < tr.n_lds; k++) {
      const uint32_t g = desc[desc[n + k]];
      rw_lds = std::max(rw_lds, lgc::region_words(0, D, cs.nv(g), lgc::tail(lds_total, image(g), (uint32_t)D)));
    }
  }
  const uint64_t glob_words = wit::glob_words(tr.glob_v);
  const uint64_t rw_glob = lgc::region_words(glob_words, D, tr.glob_v, lgc::Tail{0u, 0u, 0u});
  const uint32_t cap = c->opt.kl_grid;
  uint64_t r_lds = klabel::region_grid(res_lds, rw_lds), r_glob = klabel::region_grid(2ull * cs.dc.n_cu, rw_glob);
  if (cap) r_lds = std::min<uint64_t>(r_lds, cap), r_glob = std::min<uint64_t>(r_glob, cap);
  const uint64_t slots = gcuts::table_slots(D);
  {
    const uint64_t need[7] = {K + 1, std::max<uint64_t>(T, 1), slots + 1, slots, 2 * (uint64_t)n, 4,
                              std::max<uint64_t>(1, std::max<uint64_t>(tr.n_lds ? r_lds * rw_lds : 0ull, tr.n_glob ? r_glob * rw_glob : 0ull))};
    if ((rc = grow_group(c, need, cs.d_lgoff, cs.d_lggrow, cs.d_lgkey, cs.d_lgval, cs.d_lgdesc, cs.d_lg.ctr, cs.d_lgreg))) return rc;
  }
  cs.lg_off = gcuts::offsets32(group_off, n_groups);
  // (the call ends behind a wait for the stream: the caller's array outlives the copy)
  HIPCHK(c, hipMemcpyAsync(cs.d_lgoff.p, cs.lg_off.data(), (K + 1) * 4, hipMemcpyHostToDevice, s));
  if (T) HIPCHK(c, hipMemcpyAsync(cs.d_lggrow.p, group_labels + group_off[0], T * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(cs.d_lgdesc.p, desc.data(), 2 * n * 4, hipMemcpyHostToDevice, s));
  nemo::launch_zero(cs.d_lgkey.p, 4 * (slots + 1), s);  // the keys and, behind them, the rows handed out
  double bytes = 0, ops = 0;
  {  // the label -> row table and the groups as rows: nemo_min_group_cuts' kernels
    nemo::GcArgs ga{};
    ga.r.key = cs.d_lgkey.p, ga.r.val = cs.d_lgval.p, ga.r.slots = slots;
    ga.grow = cs.d_lggrow.p, ga.n_named = (uint32_t)T, ga.n_dist = (uint32_t)D, ga.n_rows = cs.d_lgkey.p + slots;
    const double b = 16.0 * (double)T;  // a label read, a key and a row written, the probe; per kernel
    if ((rc = timed(c, "k_gc_table", b, 0, [&] { nemo::launch_gc_table(ga, s); }))) return rc;
    if ((rc = timed(c, "k_gc_rows", b, 0, [&] { nemo::launch_gc_rows(ga, s); }))) return rc;
    bytes += 2.0 * b + 4.0 * (double)slots;
  }
  nemo::LgcArgs a{};
  nemo::LinArgs &l = a.l;
  l.region = cs.d_lgreg.p;
  a.goff = cs.d_lgoff.p, a.grow = cs.d_lggrow.p, a.n_dist = (uint32_t)D;
  a.key = cs.d_lgkey.p, a.val = cs.d_lgval.p, a.slots = slots;
  a.graph = cs.d_lgdesc.p, a.sinks = (flags & NEMO_KL_SINKS) ? 1u : 0u, a.n = (uint32_t)n, a.q = q;
  // the byte model of a level's evaluation: a work item reads its graph's image (wit_host.h) and its 4 V labels twice
  // (count, scatter); a chunk reads its 64 sets (16 bytes each) and their groups' rows, and writes a lost word; the
  // global tier adds 32 V per chunk for its two word arrays; the children are not known at the launch and are left
  // out; ops = 2 E child words per chunk, one sweep up and one pass down
  const double per_group = 8.0 + 4.0 * (double)T / (double)K;
  auto prepare = [&](uint32_t, uint64_t, uint64_t ck) -> int {
    if (int e = grow_drop(c, cs.d_lglost, (uint64_t)n * ck)) return e;
    a.lost = cs.d_lglost.p, a.n_lost = cs.d_lgnl.p;
    return NEMO_OK;
  };
  auto evaluate = [&](int pass, double *by, double *op) -> int {
    const uint64_t n_front = l.n_front, ck = l.n_chunks;
    const uint32_t d = l.size;
    for (int tier = 0; tier < 2; tier++) {
      const uint32_t nt = tier ? tr.n_glob : tr.n_lds;
      if (!nt) continue;
      const uint64_t res = tier ? r_glob : r_lds;
      const klabel::Split sp = klabel::split(nt, ck, res);
      const uint32_t grid = klabel::grid(sp.items, res, cap);
      double b = 0, o = 0;
      for (uint32_t k = 0; k < nt; k++) {
        const uint32_t g = desc[desc[n + (tier ? tr.n_lds : 0) + k]];
        const double V = (double)cs.nv(g), E = (double)cs.ne(g), L = (double)cs.kl_nlev[g];
        b += sp.parts * (wit::image_bytes(V, E, L) + 8.0 * V) + 16.0 * (double)n_front + 64.0 * d * per_group * (double)ck +
             (double)ck * (8.0 + (tier ? 32.0 * V : 0.0));
        o += (double)ck * 2.0 * E;
      }
      a.pos = cs.d_lgdesc.p + n + (tier ? tr.n_lds : 0);
      a.n_tier = nt, a.parts = sp.parts;
      l.lds_total = tier ? 0u : lds_total;
      l.region_words = tier ? rw_glob : rw_lds;
      a.glob_words = tier ? glob_words : 0;
      int e;
      if (tier) e = timed(c, "k_lgc_glob", b, o, [&] { nemo::launch_lgc_glob(cs.dc, a, grid, s); });
      else e = timed(c, "k_lgc_lds", b, o, [&] { nemo::launch_lgc_lds(cs.dc, a, grid, s); });
      if (e) return e;
      *by += b, *op += o;
    }
    if (pass) return NEMO_OK;  // the cuts of the level; a second pass finds them in place
    const double bc = 8.0 * (double)n * (double)ck + 16.0 * (double)n_front;
    *by += bc;
    return timed(c, "k_lgc_cuts", bc, 0, [&] { nemo::launch_lgc_cuts(a, s); });
  };
  auto emit_bound = [&](uint64_t n_front, uint32_t d) { return lgc::emit_bound(n, n_front, K, d); };
  uint64_t n_cuts = 0;
  if ((rc = lin_levels(c, who, "group list or the run list", cs.d_lg, c->h_lgc, c->ev_lgc, l, K, max_size, cs.lg_stats, &cs.d_lgnl, level_limit,
                       prepare, evaluate, emit_bound, &bytes, &ops, &n_cuts)))
    return rc;
  timer.done(bytes, ops);
  // the rows, sorted by (size, colex), and their counts
  LinCuts cuts;
  if ((rc = lin_sorted_keys(c, cs.d_lg, &cs.d_lgnl, c->h_lgc, c->ev_lgc, n_cuts, &cuts))) return rc;
  cs.lg_rows.resize(n_cuts);
  cs.lg_nlost.resize(n_cuts);
  for (uint64_t i = 0; i < n_cuts; i++) {
    nemo_lineage_group_cut &row = cs.lg_rows[i];
    uint32_t pos[LIN_MAX_SIZE];
    row.size = lin::key_unpack(cuts.keys[cuts.order[i]], pos);
    for (uint32_t j = 0; j < LIN_MAX_SIZE; j++) row.group[j] = j < row.size ? pos[j] : 0xFFFFFFFFu;
    cs.lg_nlost[i] = cuts.col[cuts.order[i]];
  }
  cs.lg_done = true;
  return NEMO_OK;
}

int nemo_fetch_lineage_group_cuts(nemo_ctx *c, nemo_lineage_group_cut *out, uint32_t *n_lost, uint64_t cap, uint64_t *n_out) {
  if (!c) return NEMO_ERR_INVALID;
  const std::vector<nemo_lineage_group_cut> &rows = c->cs.lg_rows;
  const int rc = fetch_result(c, c->cs.lg_done, "nemo_fetch_lineage_group_cuts", "nemo_lineage_group_cuts", rows.data(), rows.size(),
                              sizeof(nemo_lineage_group_cut), out, cap, n_out);
  if (rc == NEMO_OK && out && n_lost && !rows.empty()) memcpy(n_lost, c->cs.lg_nlost.data(), rows.size() * sizeof(uint32_t));  // the second column
  return rc;
}

int nemo_fetch_lineage_group_cut_stats(nemo_ctx *c, uint64_t out[18]) {
  if (!c || !out) return NEMO_ERR_INVALID;
  return fetch_result(c, c->cs.lg_done, "nemo_fetch_lineage_group_cut_stats", "nemo_lineage_group_cuts", c->cs.lg_stats, 18, 8, out, 18, nullptr);
}

}  // extern "C"
