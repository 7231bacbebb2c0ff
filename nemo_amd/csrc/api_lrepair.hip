// api_lrepair.hip — nemo_lineage_repair_sets, nemo_lineage_repairs and their fetches (k_lrepair.hip, lrep_host.h;
// DESIGN.md §Lineage repair search).  The calls keep their entry checks, their 65535-candidate limit and their early
// ends; the absent set and the candidates reach the device through repair_api.h's front end, shared with the
// exhaustive repair calls (api_repair.hip), on the calls' own state; the search from there to the rows is lin_api.h's
// lin_node_search, shared with nemo_lineage_cuts, with the repairs where that keeps its cuts, and the status decided
// before the levels from k_lrep_*'s two-hypothesis launch by repair_host.h's rules.  The tier rule and image are
// lrep_host.h's under the witness calls' option.
#include "knock_api.h"
#include "lin_api.h"
#include "repair_api.h"

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

// The search over graph g with the bitmap in lr_abs.d_bits and the candidates cs.lr_cand in d_lrcand (both queued on
// the stream), L Kahn levels and n_absent absent nodes.  The two-hypothesis launch decides the status; a status other
// than SEARCHED ends the call before the levels.
int lrep_search(nemo_ctx *c, const char *who, uint32_t g, uint32_t max_size, uint32_t L, uint64_t n_absent, GroupTimer &timer, double bytes) {
  CorpusState &cs = c->cs;
  hipStream_t s = c->stream;
  if (L == 0) {  // no level, no root: nothing is lost
    timer.done(bytes, 0);
    return lrep_end(c, REPAIR_HOLDS, n_absent);
  }
  LinSearch ls{who, g, max_size, lrep::lds_fits, lrep::lrep_lds_bytes, lrep::glob_words, lrep::image_bytes, nemo::lrep_lds_resident, "k_lrep_lds",
               "k_lrep_glob"};
  ls.glob_node_bytes = 48.0, ls.stats = cs.lr_stats + 2;  // the dead, the blame and the stop rule's words
  const uint64_t *absent = cs.lr_abs.d_bits.p;
  auto launch_on = [&](const nemo::LrepArgs &ra, bool lds, uint32_t grid) {
    if (lds) nemo::launch_lrep_lds(cs.dc, ra, grid, s);
    else nemo::launch_lrep_glob(cs.dc, ra, grid, s);
  };
  auto launch = [&](const nemo::LinArgs &a, bool lds, uint32_t grid) { launch_on(nemo::LrepArgs{a, absent, 0u}, lds, grid); };
  // The status, before the levels: one workgroup, S = {} and S = cand; the image read once, the candidates, the global
  // tier's three word arrays filled, the lost word written.  SEARCHED: the call's status and |A| are set and the levels
  // run; any other status ends the call here.
  auto status = [&](const nemo::LinArgs &a, bool lds, double *by, double *op, int *rc) {
    const double V = (double)cs.nv(g), E = (double)cs.ne(g);
    const double b = lrep::image_bytes(V, E, (double)L) + 4.0 * (double)a.K + (lds ? 0.0 : 24.0 * V) + 8.0, o = E;
    *by += b, *op += o;
    if ((*rc = timed(c, lds ? ls.lds_name : ls.glob_name, b, o, [&] { launch_on(nemo::LrepArgs{a, absent, 1u}, lds, 1); }))) return true;
    nemo::launch_to_host(c->h_lrep.p, a.ctr + 3, 8, s);
    if ((*rc = wait_copied(c, c->ev_lrep))) return true;
    const uint32_t st = lrep::status_of_lost(c->h_lrep.p[0]);
    if (st == REPAIR_SEARCHED) {
      cs.lr_stats[0] = st, cs.lr_stats[1] = n_absent;
      return false;
    }
    timer.done(*by, *op);
    *rc = lrep_end(c, st, n_absent);
    return true;
  };
  std::fill(cs.lr_stats, cs.lr_stats + 20, 0ull);  // the levels that do not run stay 0
  const int rc = lin_node_search(c, ls, cs.d_lr, cs.d_lrreg, cs.d_lrcand, cs.lr_cand, c->h_lrep, c->ev_lrep, L, timer, bytes, &cs.lr_rows, launch,
                                 status);
  if (rc == NEMO_OK) cs.lr_done = true;  // searched, or ended by the status (lrep_end)
  return rc;
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
  if ((rc = absent_check(c, who, absent, n_absent, cand, n_cand, cs.nv(g)))) return rc;
  const uint64_t K = cand ? n_cand : n_absent;
  if (!lrep::cands_fit(K)) return lrep_limit(c, who, K, cand ? "candidates" : "absent nodes as candidates");
  cs.lr_cand.assign(cand ? cand : absent, (cand ? cand : absent) + K);
  if (n_absent == 0) return lrep_end(c, REPAIR_HOLDS, 0);  // nothing is lost
  if ((rc = ensure_event(c, &c->ev_lrep))) return rc;
  if ((rc = c->h_lrep.grow(c, 8))) return rc;
  GroupTimer timer(c, "k_lrepair");
  uint32_t L;
  if ((rc = absent_queue(c, cs.lr_abs, cs.d_lrcand, cs.lr_cand, c->h_lrep, c->ev_lrep, g, absent, n_absent, &L))) return rc;
  return lrep_search(c, who, g, max_size, L, n_absent, timer, 0.0);
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
  cs.lr_cand.clear();
  if (cs.nv(g) == 0) return lrep_end(c, REPAIR_HOLDS, 0);
  if ((rc = ensure_event(c, &c->ev_lrep))) return rc;
  if ((rc = c->h_lrep.grow(c, 8))) return rc;
  GroupTimer timer(c, "k_lrepair");
  double bytes = 0;
  uint64_t K;
  uint32_t L;
  if ((rc = absent_pair(c, who, cs.lr_abs, cs.d_lrcand, c->h_lrep, c->ev_lrep, g, go, &bytes, &K, &L))) return rc;
  if (K == 0) {  // every sink goal's label is a goal label of the other run
    timer.done(bytes, 0);
    return lrep_end(c, REPAIR_HOLDS, 0);
  }
  if (!lrep::cands_fit(K)) return lrep_limit(c, who, K, "absent sink goals as candidates");
  // the rows name nodes: the device-made list to the host
  if ((rc = c->h_lrep.grow(c, K / 2 + 8))) return rc;
  nemo::launch_to_host(c->h_lrep.p, cs.d_lrcand.p, 4 * K, c->stream);
  if ((rc = wait_copied(c, c->ev_lrep))) return rc;
  const uint32_t *hc = reinterpret_cast<const uint32_t *>(c->h_lrep.p);
  cs.lr_cand.assign(hc, hc + K);
  return lrep_search(c, who, g, max_size, L, K, timer, bytes);
}

int nemo_fetch_lineage_repairs(nemo_ctx *c, nemo_lineage_repair *out, uint64_t cap, uint64_t *n_out) {
  if (!c) return NEMO_ERR_INVALID;
  const std::vector<nemo_lineage_repair> &rows = c->cs.lr_rows;
  return fetch_result(c, c->cs.lr_done, "nemo_fetch_lineage_repairs", LREP_CALLS, rows.data(), rows.size(), sizeof(nemo_lineage_repair), out, cap,
                      n_out);
}

int nemo_fetch_lineage_repair_stats(nemo_ctx *c, uint64_t out[20]) {
  if (!c || !out) return NEMO_ERR_INVALID;
  return fetch_result(c, c->cs.lr_done, "nemo_fetch_lineage_repair_stats", LREP_CALLS, c->cs.lr_stats, 20, 8, out, 20, nullptr);
}

int nemo_fetch_lineage_repair_cands(nemo_ctx *c, uint32_t *out, uint64_t cap, uint64_t *n_out) {
  if (!c) return NEMO_ERR_INVALID;
  const std::vector<uint32_t> &cand = c->cs.lr_cand;
  return fetch_result(c, c->cs.lr_done, "nemo_fetch_lineage_repair_cands", LREP_CALLS, cand.data(), cand.size(), 4, out, cap, n_out);
}

}  // extern "C"
