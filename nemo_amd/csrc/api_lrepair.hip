// api_lrepair.hip — nemo_lineage_repair_sets, nemo_lineage_repairs and their fetches (k_lrepair.hip, lrep_host.h;
// DESIGN.md §Lineage repair search).  The entry checks, the absent set and the candidate source are the exhaustive
// repair calls' (api_repair.hip), on the calls' own buffers; the status comes from k_lrep_*'s two-hypothesis launch by
// repair_host.h's rules; the levels are lin_api.h's lin_levels, reached through lin_run.h's lin_levels_run, with the
// repairs where those keep their cuts.  The tier rule and image are lrep_host.h's under the witness calls' option; the
// launch's dynamic LDS, the wait for the copies, the buffer group and the timing group are knock_api.h's and ctx.h's.
#include "knock_api.h"
#include "lin_run.h"

namespace {

const char *const LREP_CALLS = "nemo_lineage_repair_sets / nemo_lineage_repairs";

// the checks both entry points start with; the calls' result is void from the loaded-corpus check on
int lrep_begin(nemo_ctx *c, const char *who, const int *cond, uint32_t max_size, uint32_t flags) {
  if (c && c->node) return fail(c, NEMO_ERR_STATE, "%s: single-device contexts only (a node context does not fan it out)", who);
  if (!c) return NEMO_ERR_INVALID;
  if (!c->cs.loaded) return fail(c, NEMO_ERR_STATE, "%s without a loaded corpus (the last load failed?)", who);
  c->cs.lr_done = false;
  if (cond && *cond != 0 && *cond != 1) return fail(c, NEMO_ERR_INVALID, "%s: cond must be 0 (pre) or 1 (post)", who);
  if (!lin::size_ok(max_size, flags))
    return fail(c, NEMO_ERR_INVALID, "%s: max_size must be 1..8 and flags 0 (max_size %u, flags %#x)", who, max_size, flags);
  return NEMO_OK;
}

// a call that ends before the levels: its status, |A| and no rows; every level stat is 0
int lrep_end(nemo_ctx *c, uint32_t status, uint64_t n_absent) {
  CorpusState &cs = c->cs;
  std::fill(cs.lr_stats, cs.lr_stats + 20, 0ull);
  cs.lr_stats[0] = status, cs.lr_stats[1] = n_absent;
  cs.lr_rows.clear();
  cs.lr_done = true;
  return NEMO_OK;
}

int lrep_limit(nemo_ctx *c, const char *who, uint64_t K, const char *what) {
  return fail(c, NEMO_ERR_LIMIT, "%s: %llu %s exceed 65535 (a set is eight u16 candidate positions): shorten the candidate list", who,
              (unsigned long long)K, what);
}

// The search over graph g with the bitmap in d_lrbits and the K candidates in d_lrcand (both queued on the stream) and
// in cs.lr_cand, L Kahn levels and n_absent absent nodes.  The two-hypothesis launch decides the status; a status
// other than SEARCHED ends the call before the levels.
int lrep_search(nemo_ctx *c, const char *who, uint32_t g, uint32_t max_size, uint64_t K, uint32_t L, uint64_t n_absent, GroupTimer &timer,
                double bytes) {
  CorpusState &cs = c->cs;
  hipStream_t s = c->stream;
  const uint64_t V = cs.nv(g), E = cs.ne(g);
  int rc;
  double ops = 0;
  if (L == 0) {  // no level, no root: nothing is lost
    timer.done(bytes, 0);
    return lrep_end(c, REPAIR_HOLDS, n_absent);
  }
  // the tier and the grid: as many workgroups as are resident, at most one per chunk
  const bool lds = lrep::lds_fits(V, E, L, c->opt.wit_lds_max);
  const uint32_t image = lds ? lrep::lrep_lds_bytes((uint32_t)V, (uint32_t)E, L) : 0u;
  const uint64_t rw = lds ? 0 : lrep::glob_words(V);
  uint32_t lds_total = 0, res_lds = 1;
  if (lds && (rc = ko_lds_total(c, who, "k_lrep_lds", [&](uint32_t b) { return nemo::lrep_lds_resident(b, cs.dc.n_cu); }, image, 0, 4096,
                                &lds_total, &res_lds)))
    return rc;
  const uint32_t cap = c->opt.kl_grid;
  const uint64_t resident = lds ? res_lds : klabel::region_grid(2ull * cs.dc.n_cu, rw);
  {
    const uint64_t need[2] = {4, std::max<uint64_t>(1, rw * lin::grid(~0ull, resident, cap))};
    if ((rc = grow_group(c, need, cs.d_lr.ctr, cs.d_lrreg))) return rc;
  }
  nemo::LrepArgs a{};
  a.l.graph = g, a.l.cand = cs.d_lrcand.p, a.l.K = (uint32_t)K;
  a.l.lds_total = lds_total, a.l.region = cs.d_lrreg.p, a.l.region_words = rw;
  a.l.ctr = cs.d_lr.ctr.p;
  a.absent = cs.d_lrbits.p;
  const double img = lrep::image_bytes((double)V, (double)E, (double)L);
  {  // the status: one workgroup, S = {} and S = cand
    a.status = 1u;
    const double b = img + 4.0 * (double)K + (lds ? 0.0 : 24.0 * (double)V) + 8.0, o = (double)E;
    bytes += b, ops += o;
    if ((rc = lds ? timed(c, "k_lrep_lds", b, o, [&] { nemo::launch_lrep_lds(cs.dc, a, 1, s); })
                  : timed(c, "k_lrep_glob", b, o, [&] { nemo::launch_lrep_glob(cs.dc, a, 1, s); })))
      return rc;
    a.status = 0u;
    nemo::launch_to_host(c->h_lrep.p, cs.d_lr.ctr.p + 3, 8, s);
    if ((rc = wait_copied(c, c->ev_lrep))) return rc;
    const uint32_t status = lrep::status_of_lost(c->h_lrep.p[0]);
    if (status != REPAIR_SEARCHED) {
      timer.done(bytes, ops);
      return lrep_end(c, status, n_absent);
    }
  }
  auto level_limit = [&](uint64_t n_front, uint32_t d) -> int {
    if (lin::front_fits(n_front)) return NEMO_OK;
    return fail(c, NEMO_ERR_LIMIT, "%s: a frontier of %llu sets of size %u exceeds 2^32 - 2: shorten the candidate list", who,
                (unsigned long long)n_front, d);
  };
  auto evaluate = [&](int, double *by, double *op) -> int {
    const uint64_t ck = a.l.n_chunks;
    const uint32_t grid = lin::grid(ck, resident, cap);
    // the byte model: api_lineage.hip's, with the bitmap in the image a workgroup reads once; the global tier adds
    // 48 V per chunk for its three word arrays
    const double b = grid * img + 16.0 * (double)a.l.n_front + (lds ? 0.0 : (double)ck * 48.0 * (double)V), o = (double)ck * 2.0 * (double)E;
    *by += b, *op += o;
    if (lds) return timed(c, "k_lrep_lds", b, o, [&] { nemo::launch_lrep_lds(cs.dc, a, grid, s); });
    return timed(c, "k_lrep_glob", b, o, [&] { nemo::launch_lrep_glob(cs.dc, a, grid, s); });
  };
  auto emit_bound = [&](uint64_t n_front, uint32_t d) { return lin::emit_bound(n_front, K, d); };
  uint64_t n_rep = 0;
  std::fill(cs.lr_stats, cs.lr_stats + 20, 0ull);
  LinRun run{who, "candidate list", &cs.d_lr, &c->h_lrep, c->ev_lrep, &a.l, K, max_size, cs.lr_stats + 2, level_limit, evaluate, emit_bound};
  if ((rc = lin_levels_run(c, run, &bytes, &ops, &n_rep))) return rc;
  timer.done(bytes, ops);
  // the rows, sorted by (size, colex)
  std::vector<lin::Key> keys;
  std::vector<uint32_t> order;
  if ((rc = lin_sorted_run(c, cs.d_lr, c->h_lrep, c->ev_lrep, n_rep, &keys, &order))) return rc;
  cs.lr_rows.resize(n_rep);
  for (uint64_t i = 0; i < n_rep; i++) {
    nemo_lineage_repair &row = cs.lr_rows[i];
    uint32_t pos[LIN_MAX_SIZE];
    row.size = lin::key_unpack(keys[order[i]], pos);
    for (uint32_t j = 0; j < LIN_MAX_SIZE; j++) row.node[j] = j < row.size ? cs.lr_cand[pos[j]] : 0xFFFFFFFFu;
  }
  cs.lr_stats[0] = REPAIR_SEARCHED, cs.lr_stats[1] = n_absent;
  cs.lr_done = true;
  return NEMO_OK;
}

// a fetch of the last call's host data (no ensure_whole: no graph is read)
int lrep_fetch(nemo_ctx *c, const char *who, const void *src, uint64_t n, size_t elem, void *out, uint64_t cap, uint64_t *n_out) {
  if (c->node || !c->cs.lr_done) return fail(c, NEMO_ERR_STATE, "%s before %s (or after a later nemo_load_corpus)", who, LREP_CALLS);
  if (n_out) *n_out = n;
  if (!out) return NEMO_OK;
  if (cap < n) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  if (n) memcpy(out, src, n * elem);
  return NEMO_OK;
}

}  // namespace

extern "C" {

int nemo_lineage_repair_sets(nemo_ctx *c, uint32_t iteration, int cond, const uint32_t *absent, size_t n_absent, const uint32_t *cand,
                             size_t n_cand, uint32_t max_size, uint32_t flags) {
  const char *who = "nemo_lineage_repair_sets";
  int rc;
  if ((rc = lrep_begin(c, who, &cond, max_size, flags))) return rc;
  CorpusState &cs = c->cs;
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
  if (!lrep::cands_fit(K)) return lrep_limit(c, who, K, cand ? "candidates" : "absent nodes as candidates");
  cs.lr_cand.assign(cand ? cand : absent, (cand ? cand : absent) + K);
  if (n_absent == 0) return lrep_end(c, REPAIR_HOLDS, 0);  // nothing is lost
  if ((rc = ensure_event(c, &c->ev_lrep))) return rc;
  if ((rc = c->h_lrep.grow(c, 8))) return rc;
  hipStream_t s = c->stream;
  GroupTimer timer(c, "k_lrepair");
  {
    const uint64_t need[2] = {repair::bitmap_words(V), std::max<uint64_t>(K, 1)};
    if ((rc = grow_group(c, need, cs.d_lrbits, cs.d_lrcand))) return rc;
  }
  cs.lr_bits = repair::bitmap(absent, n_absent, V);
  HIPCHK(c, hipMemcpyAsync(cs.d_lrbits.p, cs.lr_bits.data(), 8 * cs.lr_bits.size(), hipMemcpyHostToDevice, s));
  if (K) HIPCHK(c, hipMemcpyAsync(cs.d_lrcand.p, cs.lr_cand.data(), 4 * K, hipMemcpyHostToDevice, s));
  nemo::launch_to_host(c->h_lrep.p, cs.dc.nlev + g, 4, s);  // the graph's Kahn level count, for the tier
  if ((rc = wait_copied(c, c->ev_lrep))) return rc;
  const uint32_t L = reinterpret_cast<const uint32_t *>(c->h_lrep.p)[0];
  return lrep_search(c, who, g, max_size, K, L, n_absent, timer, 0.0);
}

// The pair form: A = cand = the sink goals of base's post graph whose label is no goal label of other's post graph,
// made on the device by k_repair_absent as nemo_min_repairs makes them, into the calls' own buffers.
int nemo_lineage_repairs(nemo_ctx *c, uint32_t base_iter, uint32_t other_iter, uint32_t max_size, uint32_t flags) {
  const char *who = "nemo_lineage_repairs";
  int rc;
  if ((rc = lrep_begin(c, who, nullptr, max_size, flags))) return rc;
  CorpusState &cs = c->cs;
  if (!cs.marked) return fail(c, NEMO_ERR_STATE, "%s before nemo_mark_holds", who);
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_whole(c))) return rc;  // reads both graphs
  if ((rc = ensure_load_checked(c))) return rc;
  uint32_t rb, ro;
  if ((rc = run_index(c, base_iter, &rb)) || (rc = run_index(c, other_iter, &ro))) return rc;
  const uint32_t g = 2 * rb + 1, go = 2 * ro + 1;
  const uint64_t V = cs.nv(g);
  cs.lr_cand.clear();
  if (V == 0) return lrep_end(c, REPAIR_HOLDS, 0);
  const pairs::Plan plan = pairs::plan(&go, 1, cs.node_off.data(), cs.run0 >= 0 ? (int64_t)cs.g0() : -1);
  if (!plan.ok) return fail(c, NEMO_ERR_LIMIT, "%s: a label table would exceed 2^32 slots", who);
  const bool shared = plan.entry_tab[0] == PAIRS_SHARED;
  if ((rc = ensure_event(c, &c->ev_lrep))) return rc;
  if ((rc = c->h_lrep.grow(c, 8))) return rc;
  hipStream_t s = c->stream;
  GroupTimer timer(c, "k_lrepair");
  if (!cs.d_lrcnt.p || (!shared && (!cs.d_lrtab.p || plan.words > cs.d_lrhreg.cap || !cs.d_lrhreg.p))) {
    HIPCHK(c, hipStreamSynchronize(s));  // an earlier call may still use them
    if ((rc = cs.d_lrcnt.grow(c, 2))) return rc;
    if (!shared && ((rc = cs.d_lrtab.grow(c, 1)) || (rc = cs.d_lrhreg.grow(c, plan.words)))) return rc;
  }
  {
    const uint64_t need[2] = {repair::bitmap_words(V), V};
    if ((rc = grow_group(c, need, cs.d_lrbits, cs.d_lrcand))) return rc;
  }
  double bytes = 0;
  cs.lr_tab = shared ? nemo::LabTab{cs.d_r0hkey, cs.r0hmask, go} : nemo::LabTab{cs.d_lrhreg.p, plan.tab_mask[0], go};
  if (!shared) {
    HIPCHK(c, hipMemcpyAsync(cs.d_lrtab.p, &cs.lr_tab, sizeof(nemo::LabTab), hipMemcpyHostToDevice, s));
    const uint32_t lds_max = c->opt.pair_hash_lds_max;
    const uint32_t lds_slots = plan.tab_mask[0] < lds_max ? plan.tab_mask[0] + 1u : 0u;
    const double b = 8.0 * (double)plan.nodes + 4.0 * (double)plan.words;
    if ((rc = timed(c, "k_lab_hash", b, 0, [&] { nemo::launch_lab_hash(cs.dc, cs.d_lrtab.p, 1, lds_max, lds_slots, s); }))) return rc;
    bytes += b;
  }
  {
    // node word, label and two row pointers of every node, a probe per sink goal, the bitmap and the list written
    const double b = 20.0 * (double)V + (double)V / 8.0 + 8.0;
    if ((rc = timed(c, "k_repair_absent", b, 0, [&] {
           nemo::launch_repair_absent(cs.dc, g, cs.lr_tab.key, cs.lr_tab.mask, cs.d_lrbits.p, cs.d_lrcand.p, cs.d_lrcnt.p, s);
         })))
      return rc;
    bytes += b;
  }
  nemo::launch_to_host(c->h_lrep.p, cs.d_lrcnt.p, 8, s);  // the count beside the Kahn level count
  if ((rc = wait_copied(c, c->ev_lrep))) return rc;
  const uint64_t K = reinterpret_cast<const uint32_t *>(c->h_lrep.p)[0];
  const uint32_t L = reinterpret_cast<const uint32_t *>(c->h_lrep.p)[1];
  if (K == 0) {  // every sink goal's label is a goal label of the other run
    timer.done(bytes, 0);
    return lrep_end(c, REPAIR_HOLDS, 0);
  }
  if (!lrep::cands_fit(K)) return lrep_limit(c, who, K, "absent sink goals as candidates");
  // the rows name nodes: the device-made list to the host
  if ((rc = c->h_lrep.grow(c, K / 2 + 8))) return rc;
  nemo::launch_to_host(c->h_lrep.p, cs.d_lrcand.p, 4 * K, s);
  if ((rc = wait_copied(c, c->ev_lrep))) return rc;
  const uint32_t *hc = reinterpret_cast<const uint32_t *>(c->h_lrep.p);
  cs.lr_cand.assign(hc, hc + K);
  return lrep_search(c, who, g, max_size, K, L, K, timer, bytes);
}

int nemo_fetch_lineage_repairs(nemo_ctx *c, nemo_lineage_repair *out, uint64_t cap, uint64_t *n_out) {
  if (!c) return NEMO_ERR_INVALID;
  return lrep_fetch(c, "nemo_fetch_lineage_repairs", c->cs.lr_rows.data(), c->cs.lr_rows.size(), sizeof(nemo_lineage_repair), out, cap, n_out);
}

int nemo_fetch_lineage_repair_stats(nemo_ctx *c, uint64_t out[20]) {
  if (!c || !out) return NEMO_ERR_INVALID;
  return lrep_fetch(c, "nemo_fetch_lineage_repair_stats", c->cs.lr_stats, 20, 8, out, 20, nullptr);
}

int nemo_fetch_lineage_repair_cands(nemo_ctx *c, uint32_t *out, uint64_t cap, uint64_t *n_out) {
  if (!c) return NEMO_ERR_INVALID;
  return lrep_fetch(c, "nemo_fetch_lineage_repair_cands", c->cs.lr_cand.data(), c->cs.lr_cand.size(), 4, out, cap, n_out);
}

}  // extern "C"
