// api_lineage.hip — nemo_lineage_cuts and its fetches (k_lineage.hip, lin_host.h; DESIGN.md §Lineage-driven cut
// search).  The level counts, the tier rule and image (wit_host.h: the witness calls'), the launch's dynamic LDS, the
// wait for the copies, the buffer group and the timing group are knock_api.h's and ctx.h's, shared with the knock-out
// family.  The host drives the levels: per level it queues the evaluation and the filter, reads one block of three
// counters from pinned memory, and decides whether the level runs again behind a grown emission buffer.
#include "knock_api.h"

namespace {

int lin_empty(CorpusState &cs) {  // zero rows, every stat 0
  cs.lin_done = true;
  return NEMO_OK;
}

}  // namespace

extern "C" {

int nemo_lineage_cuts(nemo_ctx *c, uint32_t iteration, int cond, const uint32_t *cand, size_t n_cand, uint32_t max_size,
                      uint32_t flags) {
  static const char *const who = "nemo_lineage_cuts";
  if (c && c->node)
    return fail(c, NEMO_ERR_STATE, "nemo_lineage_cuts: single-device contexts only (a node context does not fan it out)");
  if (!c) return NEMO_ERR_INVALID;
  CorpusState &cs = c->cs;
  if (!cs.loaded) return fail(c, NEMO_ERR_STATE, "nemo_lineage_cuts without a loaded corpus (the last load failed?)");
  cs.lin_done = false;
  if (cond != 0 && cond != 1) return fail(c, NEMO_ERR_INVALID, "nemo_lineage_cuts: cond must be 0 (pre) or 1 (post)");
  if (!lin::size_ok(max_size, flags))
    return fail(c, NEMO_ERR_INVALID, "nemo_lineage_cuts: max_size must be 1..8 and flags 0 (max_size %u, flags %#x)", max_size, flags);
  if (cand && n_cand > LIN_MAX_CAND)  // before the list is read
    return fail(c, NEMO_ERR_LIMIT, "nemo_lineage_cuts: %zu candidates exceed 65535 (a set is eight u16 candidate positions): shorten the candidate list",
                n_cand);
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
    switch (lin::check_cands(cand, n_cand, V, &where)) {
      case lin::CAND_RANGE:
        return fail(c, NEMO_ERR_INVALID, "nemo_lineage_cuts: candidate %zu is node %u, out of range (%llu nodes)", where, cand[where],
                    (unsigned long long)V);
      case lin::CAND_DUP:
        return fail(c, NEMO_ERR_INVALID, "nemo_lineage_cuts: candidate %zu names node %u a second time", where, cand[where]);
      default:
        break;
    }
  }
  std::fill(cs.lin_stats, cs.lin_stats + 18, 0ull);
  cs.lin_rows.clear();
  if (cand && n_cand == 0) return lin_empty(cs);
  if (V == 0) return lin_empty(cs);  // no node, no root
  if ((rc = ensure_event(c, &c->ev_lin))) return rc;
  hipStream_t s = c->stream;
  if ((rc = ensure_nlev(c, c->h_lin, c->ev_lin))) return rc;
  const uint32_t L = cs.kl_nlev[g];
  if (L == 0) return lin_empty(cs);
  if ((rc = c->h_lin.grow(c, 8))) return rc;
  GroupTimer timer(c, "k_lineage");
  double bytes = 0, ops = 0;
  if ((rc = grow_drop(c, cs.d_lndesc, 8))) return rc;
  // cand == NULL: the graph's sink goals, counted by k_ko_leaves
  uint32_t *desc = cs.d_lndesc.p;  // [0] the graph | [1..2] offsets 0, K | [4..5] (sink goals, Kahn levels)
  nemo::KnockArgs ka{};
  ka.list = desc, ka.loff = desc + 1, ka.cnt = desc + 4, ka.n_list = 1;
  uint64_t K = n_cand;
  if (!cand) {
    cs.lin_up[0] = g, cs.lin_up[1] = 0u;
    HIPCHK(c, hipMemcpyAsync(desc, cs.lin_up, 8, hipMemcpyHostToDevice, s));
    const double b_leaves = 8.0 * (double)V + 12.0;
    if ((rc = timed(c, "k_ko_leaves", b_leaves, 0, [&] { nemo::launch_ko_leaves(cs.dc, ka, false, s); }))) return rc;
    nemo::launch_to_host(c->h_lin.p, ka.cnt, 8, s);
    if ((rc = wait_copied(c, c->ev_lin))) return rc;
    K = reinterpret_cast<const uint32_t *>(c->h_lin.p)[0];
    bytes += b_leaves;
    if (K > LIN_MAX_CAND)
      return fail(c, NEMO_ERR_LIMIT, "nemo_lineage_cuts: %llu sink goals exceed 65535 candidates (a set is eight u16 candidate positions): pass a list",
                  (unsigned long long)K);
  }
  // the tier and the grid: as many workgroups as are resident, at most one per chunk
  const bool lds = wit::lds_fits(V, E, L, c->opt.wit_lds_max);
  const uint32_t image = lds ? wit::wit_lds_bytes((uint32_t)V, (uint32_t)E, L) : 0u;
  const uint64_t rw = lds ? 0 : wit::glob_words(V);
  uint32_t lds_total = 0, res_lds = 1;
  if (lds && (rc = ko_lds_total(c, who, "k_lin_lds", [&](uint32_t b) { return nemo::lin_lds_resident(b, cs.dc.n_cu); }, image, 0, 4096,
                                &lds_total, &res_lds)))
    return rc;
  const uint32_t cap = c->opt.kl_grid;
  const uint64_t resident = lds ? res_lds : klabel::region_grid(2ull * cs.dc.n_cu, rw);
  {
    const uint64_t need[3] = {std::max<uint64_t>(K, 1), 4, std::max<uint64_t>(1, rw * lin::grid(~0ull, resident, cap))};
    if ((rc = grow_group(c, need, cs.d_lncand, cs.d_lnctr, cs.d_lnreg))) return rc;
  }
  if (cand) {
    cs.lin_cand.assign(cand, cand + K);
    if (K) HIPCHK(c, hipMemcpyAsync(cs.d_lncand.p, cs.lin_cand.data(), K * 4, hipMemcpyHostToDevice, s));
  } else if (K) {
    cs.lin_up[2] = 0u, cs.lin_up[3] = (uint32_t)K;
    HIPCHK(c, hipMemcpyAsync(desc + 1, cs.lin_up + 2, 8, hipMemcpyHostToDevice, s));
    ka.leaf = cs.d_lncand.p;
    const double b_leaves = 8.0 * (double)V + 12.0 + 4.0 * (double)K;
    if ((rc = timed(c, "k_ko_leaves", b_leaves, 0, [&] { nemo::launch_ko_leaves(cs.dc, ka, true, s); }))) return rc;
    bytes += b_leaves;
    if ((rc = c->h_lin.grow(c, K / 2 + 8))) return rc;
    nemo::launch_to_host(c->h_lin.p, cs.d_lncand.p, 4 * K, s);
    if ((rc = wait_copied(c, c->ev_lin))) return rc;
    const uint32_t *hc = reinterpret_cast<const uint32_t *>(c->h_lin.p);
    cs.lin_cand.assign(hc, hc + K);
  } else {
    cs.lin_cand.clear();
  }
  // the emission buffer (it starts small), the frontier and the children's table; the cuts' list and table
  uint64_t kids_cap = std::max<uint64_t>(cs.d_lnkids.cap / 2, LIN_EMIT_START);
  if ((rc = grow_drop(c, cs.d_lnkids, 2 * kids_cap)) || (rc = grow_drop(c, cs.d_lnktab, lin::table_slots(kids_cap))) ||
      (rc = grow_drop(c, cs.d_lnfront, 2 * kids_cap)))
    return rc;
  uint64_t cuts_cap = std::max<uint64_t>(cs.d_lncuts.cap / 2, LIN_MIN_TABLE);
  if ((rc = grow_drop(c, cs.d_lncuts, 2 * cuts_cap)) || (rc = grow_drop(c, cs.d_lnctab, lin::table_slots(cuts_cap)))) return rc;
  uint64_t cslots = lin::table_slots(cuts_cap);
  nemo::launch_zero(cs.d_lnctab.p, 4 * cslots, s);
  nemo::launch_zero(cs.d_lnctr.p, 32, s);
  {  // level 0's frontier: the empty set, every field LIN_PAD
    static const uint64_t empty[2] = {~0ull, ~0ull};
    HIPCHK(c, hipMemcpyAsync(cs.d_lnfront.p, empty, 16, hipMemcpyHostToDevice, s));
  }
  nemo::LinArgs a{};
  a.graph = g, a.cand = cs.d_lncand.p, a.K = (uint32_t)K, a.ctr = cs.d_lnctr.p;
  a.lds_total = lds_total, a.region = cs.d_lnreg.p, a.region_words = rw;
  const double img = wit::image_bytes((double)V, (double)E, (double)L);
  uint64_t n_front = 1, n_cuts = 0;
  uint32_t cut_sizes = 0;
  volatile const uint64_t *hctr = c->h_lin.p;
  for (uint32_t d = 0; d <= max_size; d++) {
    if (!lin::front_fits(n_front))
      return fail(c, NEMO_ERR_LIMIT, "nemo_lineage_cuts: a frontier of %llu sets of size %u exceeds 2^32 - 2: shorten the candidate list",
                  (unsigned long long)n_front, d);
    cs.lin_stats[2 * d] = n_front;
    const uint64_t grown = lin::cuts_grown(cuts_cap, n_cuts, n_front);
    if (grown != cuts_cap) {  // every set of the level may be a cut: the list with its contents, the table anew
      if ((rc = grow_keep(c, cs.d_lncuts, 2 * grown, 2 * n_cuts)) || (rc = grow_drop(c, cs.d_lnctab, lin::table_slots(grown)))) return rc;
      cuts_cap = grown, cslots = lin::table_slots(grown);
      nemo::launch_zero(cs.d_lnctab.p, 4 * cslots, s);
      a.cuts = cs.d_lncuts.p, a.ctab = cs.d_lnctab.p, a.cslots = cslots;
      if ((rc = timed(c, "k_lin_rehash", 20.0 * (double)n_cuts, 0, [&] { nemo::launch_lin_rehash(a, n_cuts, s); }))) return rc;
    }
    const bool emit = d < max_size;
    const uint64_t ck = lin::chunks(n_front);
    const uint32_t grid = lin::grid(ck, resident, cap);
    uint64_t counted = 0;
    for (int attempt = 0;; attempt++) {
      nemo::launch_zero(cs.d_lnctr.p + 1, 16, s);
      a.front = cs.d_lnfront.p, a.n_front = (uint32_t)n_front, a.n_chunks = (uint32_t)ck;
      a.emit = emit ? 1u : 0u, a.redo = attempt ? 1u : 0u;
      a.kids = cs.d_lnkids.p, a.kids_cap = kids_cap;
      a.cuts = cs.d_lncuts.p, a.ctab = cs.d_lnctab.p, a.cslots = cslots;
      a.next = cs.d_lnfront.p, a.cut_sizes = cut_sizes, a.size = d, a.cuts_before = n_cuts;
      // the byte model: a workgroup reads the image once (wit_host.h); a set is 16 bytes read; the global tier adds
      // 32 V per chunk for its two word arrays; the children are not known at the launch and are left out; ops = 2 E
      // child words per chunk, one sweep up and one pass down
      const double b = grid * img + 16.0 * (double)n_front + (lds ? 0.0 : (double)ck * 32.0 * (double)V), o = (double)ck * 2.0 * (double)E;
      if (lds) rc = timed(c, "k_lin_lds", b, o, [&] { nemo::launch_lin_lds(cs.dc, a, grid, s); });
      else rc = timed(c, "k_lin_glob", b, o, [&] { nemo::launch_lin_glob(cs.dc, a, grid, s); });
      if (rc) return rc;
      bytes += b, ops += o;
      if (emit) {
        const uint64_t most = std::min(kids_cap, lin::emit_bound(n_front, K, d));
        a.ktab = cs.d_lnktab.p, a.kslots = lin::table_slots(most);
        nemo::launch_zero(cs.d_lnktab.p, 4 * a.kslots, s);
        const double bf = 4.0 * (double)a.kslots;
        if ((rc = timed(c, "k_lin_filter", bf, 0, [&] { nemo::launch_lin_filter(a, lin::filter_grid(most, LIN_BLOCK, 8ull * cs.dc.n_cu), s); })))
          return rc;
        bytes += bf;
      }
      nemo::launch_to_host(c->h_lin.p, cs.d_lnctr.p, 32, s);
      if ((rc = wait_copied(c, c->ev_lin))) return rc;
      counted = hctr[1];
      if (!emit || counted <= kids_cap) break;
      if (counted > c->opt.lin_children_max) break;  // reported below
      if (attempt) return fail(c, NEMO_ERR_HIP, "nemo_lineage_cuts: level %u counted %llu children behind a buffer grown to its first count", d, (unsigned long long)counted);
      // the level overflowed: the buffer to the counted size, the frontier kept, and the level once more
      kids_cap = lin::emit_grown(kids_cap, counted);
      if ((rc = grow_drop(c, cs.d_lnkids, 2 * kids_cap)) || (rc = grow_drop(c, cs.d_lnktab, lin::table_slots(kids_cap))) ||
          (rc = grow_keep(c, cs.d_lnfront, 2 * kids_cap, 2 * n_front)))
        return rc;
    }
    if (emit && counted > c->opt.lin_children_max)
      return fail(c, NEMO_ERR_LIMIT,
                  "nemo_lineage_cuts: level %u emits %llu children, more than the option \"lineage_children_max\" allows (%llu): raise it, or shorten the candidate list",
                  d, (unsigned long long)counted, (unsigned long long)c->opt.lin_children_max);
    const uint64_t cuts_now = hctr[0];
    cs.lin_stats[2 * d + 1] = cuts_now - n_cuts;
    if (cuts_now > n_cuts) cut_sizes |= 1u << d;
    n_cuts = cuts_now;
    if (!emit) break;
    n_front = hctr[2];
    if (!n_front) break;
  }
  timer.done(bytes, ops);
  // the cuts' keys to the host; the rows sorted by (size, colex)
  std::vector<lin::Key> keys(n_cuts);
  if (n_cuts) {
    if ((rc = c->h_lin.grow(c, 2 * n_cuts))) return rc;
    nemo::launch_to_host(c->h_lin.p, cs.d_lncuts.p, 16 * n_cuts, s);
    if ((rc = wait_copied(c, c->ev_lin))) return rc;
    for (uint64_t i = 0; i < n_cuts; i++) keys[i] = lin::Key{c->h_lin.p[2 * i], c->h_lin.p[2 * i + 1]};
    std::sort(keys.begin(), keys.end(), lin::row_less);
  }
  cs.lin_rows.resize(n_cuts);
  for (uint64_t i = 0; i < n_cuts; i++) {
    nemo_lineage_cut &row = cs.lin_rows[i];
    uint32_t pos[LIN_MAX_SIZE];
    row.size = lin::key_unpack(keys[i], pos);
    for (uint32_t j = 0; j < LIN_MAX_SIZE; j++) row.node[j] = j < row.size ? cs.lin_cand[pos[j]] : 0xFFFFFFFFu;
  }
  cs.lin_done = true;
  return NEMO_OK;
}

int nemo_fetch_lineage_cuts(nemo_ctx *c, nemo_lineage_cut *out, uint64_t cap, uint64_t *n_out) {
  if (!c) return NEMO_ERR_INVALID;
  if (c->node || !c->cs.lin_done)
    return fail(c, NEMO_ERR_STATE, "nemo_fetch_lineage_cuts before nemo_lineage_cuts (or after a later nemo_load_corpus)");
  const uint64_t n = c->cs.lin_rows.size();  // no ensure_whole: reads the last call's host rows, no graph
  if (n_out) *n_out = n;
  if (!out) return NEMO_OK;
  if (cap < n) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  if (n) memcpy(out, c->cs.lin_rows.data(), n * sizeof(nemo_lineage_cut));
  return NEMO_OK;
}

int nemo_fetch_lineage_cut_stats(nemo_ctx *c, uint64_t out[18]) {
  if (!c || !out) return NEMO_ERR_INVALID;
  if (c->node || !c->cs.lin_done)
    return fail(c, NEMO_ERR_STATE, "nemo_fetch_lineage_cut_stats before nemo_lineage_cuts (or after a later nemo_load_corpus)");
  memcpy(out, c->cs.lin_stats, sizeof c->cs.lin_stats);
  return NEMO_OK;
}

}  // extern "C"
