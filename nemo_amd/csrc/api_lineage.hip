// api_lineage.hip — nemo_lineage_cuts and its fetches (k_lineage.hip, lin_host.h; DESIGN.md §Lineage-driven cut
// search).  The level counts, the tier rule and image (wit_host.h: the witness calls'), the launch's dynamic LDS, the
// wait for the copies, the buffer group and the timing group are knock_api.h's and ctx.h's, shared with the knock-out
// family.  The host drives the levels (lin_api.h's lin_levels, shared with nemo_lineage_group_cuts): per level it
// queues the evaluation and the filter, reads one block of three counters from pinned memory, and decides whether the
// level runs again behind a grown emission buffer.
#include "knock_api.h"
#include "lin_api.h"
#include "lin_run.h"

// lin_run.h: the level loop and the keys' way to the host for a search in a translation unit of its own
int lin_levels_run(nemo_ctx *c, const LinRun &r, double *bytes, double *ops, uint64_t *n_found) {
  auto prepare = [](uint32_t, uint64_t, uint64_t) { return NEMO_OK; };
  return lin_levels(c, r.who, r.shorten, *r.bufs, *r.h, r.ev, *r.a, r.K, r.max_size, r.stats, nullptr, r.level_limit, prepare, r.evaluate,
                    r.emit_bound, bytes, ops, n_found);
}

int lin_sorted_run(nemo_ctx *c, const LinBufs &b, Pinned<uint64_t> &h, hipEvent_t ev, uint64_t n, std::vector<lin::Key> *keys,
                   std::vector<uint32_t> *order) {
  LinCuts cuts;
  if (int rc = lin_sorted_keys(c, b, nullptr, h, ev, n, &cuts)) return rc;
  keys->swap(cuts.keys), order->swap(cuts.order);
  return NEMO_OK;
}

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
    if ((rc = grow_group(c, need, cs.d_lncand, cs.d_ln.ctr, cs.d_lnreg))) return rc;
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
  nemo::LinArgs a{};
  a.graph = g, a.cand = cs.d_lncand.p;
  a.lds_total = lds_total, a.region = cs.d_lnreg.p, a.region_words = rw;
  const double img = wit::image_bytes((double)V, (double)E, (double)L);
  auto level_limit = [&](uint64_t n_front, uint32_t d) -> int {
    if (lin::front_fits(n_front)) return NEMO_OK;
    return fail(c, NEMO_ERR_LIMIT, "nemo_lineage_cuts: a frontier of %llu sets of size %u exceeds 2^32 - 2: shorten the candidate list",
                (unsigned long long)n_front, d);
  };
  auto prepare = [](uint32_t, uint64_t, uint64_t) { return NEMO_OK; };  // nothing is sized by the level
  auto evaluate = [&](int, double *by, double *op) -> int {
    const uint64_t ck = a.n_chunks;
    const uint32_t grid = lin::grid(ck, resident, cap);
    // the byte model: a workgroup reads the image once (wit_host.h); a set is 16 bytes read; the global tier adds
    // 32 V per chunk for its two word arrays; the children are not known at the launch and are left out; ops = 2 E
    // child words per chunk, one sweep up and one pass down
    const double b = grid * img + 16.0 * (double)a.n_front + (lds ? 0.0 : (double)ck * 32.0 * (double)V), o = (double)ck * 2.0 * (double)E;
    *by += b, *op += o;
    if (lds) return timed(c, "k_lin_lds", b, o, [&] { nemo::launch_lin_lds(cs.dc, a, grid, s); });
    return timed(c, "k_lin_glob", b, o, [&] { nemo::launch_lin_glob(cs.dc, a, grid, s); });
  };
  auto emit_bound = [&](uint64_t n_front, uint32_t d) { return lin::emit_bound(n_front, K, d); };
  uint64_t n_cuts = 0;
  if ((rc = lin_levels(c, who, "candidate list", cs.d_ln, c->h_lin, c->ev_lin, a, K, max_size, cs.lin_stats, nullptr, level_limit, prepare, evaluate,
                       emit_bound, &bytes, &ops, &n_cuts)))
    return rc;
  timer.done(bytes, ops);
  // the rows, sorted by (size, colex)
  LinCuts cuts;
  if ((rc = lin_sorted_keys(c, cs.d_ln, nullptr, c->h_lin, c->ev_lin, n_cuts, &cuts))) return rc;
  cs.lin_rows.resize(n_cuts);
  for (uint64_t i = 0; i < n_cuts; i++) {
    nemo_lineage_cut &row = cs.lin_rows[i];
    uint32_t pos[LIN_MAX_SIZE];
    row.size = lin::key_unpack(cuts.keys[cuts.order[i]], pos);
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
