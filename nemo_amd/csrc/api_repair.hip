// api_repair.hip — nemo_min_repair_sets, nemo_min_repairs and their fetches (k_repair.hip, repair_host.h; DESIGN.md
// §Minimal repair sets).  The calls keep their entry checks and early ends; the absent set and the candidates reach
// the device through repair_api.h's front end, shared with api_lrepair.hip, on the calls' own state; the search from
// there to the rows is cut_api.h's node_search, shared with api_cuts.hip, with a round 0, the bitmap in the image
// and the status decided from round 0's word.
#include "cut_api.h"
#include "repair_api.h"

namespace {

// a call that ends before the search: its status, |A| and no rows
int repair_end(nemo_ctx *c, uint32_t status, uint64_t n_absent) {
  CorpusState &cs = c->cs;
  std::fill(cs.rp_stats, cs.rp_stats + 11, 0ull);
  cs.rp_stats[0] = status, cs.rp_stats[1] = n_absent;
  cs.rp.n_rows = 0;
  cs.rp.done = true;
  return NEMO_OK;
}

// The search over graph g with the bitmap in rp_abs.d_bits and the K candidates in rp.cand (both queued on the stream), L
// Kahn levels and n_absent absent nodes.  from_dev: rp.h_cand is not known yet (the pair form).  Round 0's word
// decides the status; a status other than SEARCHED ends the call (round 1 was wasted).
int repair_search(nemo_ctx *c, const char *who, uint32_t g, uint32_t max_size, uint64_t K, uint32_t L, uint64_t n_absent, bool from_dev,
                  GroupTimer &timer, double bytes) {
  CorpusState &cs = c->cs;
  hipStream_t s = c->stream;
  NodeSearch ns{who, g, max_size, repair::lds_fits, repair::repair_lds_bytes, nemo::repair_lds_resident, "k_repair_lds", "k_repair_glob"};
  auto launch = [&](const nemo::CutArgs &a, bool lds, uint32_t grid, uint32_t lds_bytes) {
    const nemo::RepairArgs ra{a, cs.rp_abs.d_bits.p, (uint32_t)K};
    if (lds) nemo::launch_repair_lds(cs.dc, ra, grid, lds_bytes, s);
    else nemo::launch_repair_glob(cs.dc, ra, grid, s);
  };
  // the bitmap: read once per workgroup on the LDS tier and once per chunk on the global tier, as the image
  ns.round0 = true, ns.image_extra = 8.0 * (double)repair::bitmap_words(cs.nv(g)), ns.cand_from_dev = from_dev;
  bool searched = false;
  auto decide = [&](const uint64_t *words, uint64_t ck1, double b, double ops, int *rc) {
    const uint32_t status = repair::status(words[ck1]);
    if ((searched = status == REPAIR_SEARCHED)) return false;
    timer.done(b, ops);
    *rc = repair_end(c, status, n_absent);
    return true;
  };
  std::fill(cs.rp_stats, cs.rp_stats + 11, 0ull);  // the rounds that do not run stay 0
  ns.stats = cs.rp_stats + 2;
  const int rc = node_search(c, ns, cs.rp, c->h_repair, c->ev_repair, K, L, timer, bytes, launch, decide);
  if (rc == NEMO_OK && searched) cs.rp_stats[0] = REPAIR_SEARCHED, cs.rp_stats[1] = n_absent;
  return rc;
}

}  // namespace

extern "C" {

int nemo_min_repair_sets(nemo_ctx *c, uint32_t iteration, int cond, const uint32_t *absent, size_t n_absent, const uint32_t *cand,
                         size_t n_cand, uint32_t max_size, uint32_t flags) {
  const char *who = "nemo_min_repair_sets";
  int rc;
  if ((rc = node_search_begin(c, who, &CorpusState::rp, nullptr, max_size, flags)) || (rc = node_search_cond(c, who, cond))) return rc;
  CorpusState &cs = c->cs;
  if ((!absent && n_absent) || (cand && !absent && n_cand)) return fail(c, NEMO_ERR_INVALID, "%s: a null absent list", who);
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_whole(c))) return rc;  // reads the graph's build outputs
  if ((rc = ensure_load_checked(c))) return rc;
  uint32_t r;
  if ((rc = run_index(c, iteration, &r))) return rc;
  const uint32_t g = 2 * r + (uint32_t)cond;
  const uint64_t V = cs.nv(g);
  if ((rc = absent_check(c, who, absent, n_absent, cand, n_cand, V))) return rc;
  const uint64_t K = cand ? n_cand : n_absent;
  cs.rp.h_cand.assign(cand ? cand : absent, (cand ? cand : absent) + K);
  if (n_absent == 0) return repair_end(c, REPAIR_HOLDS, 0);  // nothing is lost
  if ((rc = ensure_event(c, &c->ev_repair))) return rc;
  if ((rc = c->h_repair.grow(c, 8))) return rc;
  GroupTimer timer(c, "k_repair");
  uint32_t L;
  if ((rc = absent_queue(c, cs.rp_abs, cs.rp.cand, cs.rp.h_cand, c->h_repair, c->ev_repair, g, absent, n_absent, &L))) return rc;
  return repair_search(c, who, g, max_size, K, L, n_absent, false, timer, 0.0);
}

// The pair form: A = cand = the sink goals of base's post graph whose label is no goal label of other's post graph,
// made on the device.  The other run's table is the load's for run 0, else k_lab_hash's, as nemo_diffprov_pairs'.
int nemo_min_repairs(nemo_ctx *c, uint32_t base_iter, uint32_t other_iter, uint32_t max_size, uint32_t flags) {
  const char *who = "nemo_min_repairs";
  int rc;
  if ((rc = node_search_begin(c, who, &CorpusState::rp, nullptr, max_size, flags))) return rc;
  CorpusState &cs = c->cs;
  if (!cs.marked) return fail(c, NEMO_ERR_STATE, "%s before nemo_mark_holds", who);
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_whole(c))) return rc;  // reads both graphs
  if ((rc = ensure_load_checked(c))) return rc;
  uint32_t rb, ro;
  if ((rc = run_index(c, base_iter, &rb)) || (rc = run_index(c, other_iter, &ro))) return rc;
  const uint32_t g = 2 * rb + 1, go = 2 * ro + 1;
  const uint64_t V = cs.nv(g);
  cs.rp.h_cand.clear();
  if (V == 0) return repair_end(c, REPAIR_HOLDS, 0);
  if ((rc = ensure_event(c, &c->ev_repair))) return rc;
  if ((rc = c->h_repair.grow(c, 8))) return rc;
  GroupTimer timer(c, "k_repair");
  double bytes = 0;
  uint64_t K;
  uint32_t L;
  if ((rc = absent_pair(c, who, cs.rp_abs, cs.rp.cand, c->h_repair, c->ev_repair, g, go, &bytes, &K, &L))) return rc;
  if (K == 0) {  // every sink goal's label is a goal label of the other run
    timer.done(bytes, 0);
    return repair_end(c, REPAIR_HOLDS, 0);
  }
  return repair_search(c, who, g, max_size, K, L, K, true, timer, bytes);
}

static const char *const REPAIR_CALLS = "nemo_min_repair_sets / nemo_min_repairs";

int nemo_fetch_min_repairs(nemo_ctx *c, nemo_repair *out, uint64_t cap, uint64_t *n_out) {
  if (!c) return NEMO_ERR_INVALID;
  return fetch_result(c, c->cs.rp.done, "nemo_fetch_min_repairs", REPAIR_CALLS, c->h_repair.p, c->cs.rp.n_rows, sizeof(nemo_repair), out, cap, n_out);
}

int nemo_fetch_min_repair_stats(nemo_ctx *c, uint64_t out[11]) {
  if (!c || !out) return NEMO_ERR_INVALID;
  return fetch_result(c, c->cs.rp.done, "nemo_fetch_min_repair_stats", REPAIR_CALLS, c->cs.rp_stats, 11, 8, out, 11, nullptr);
}

int nemo_fetch_min_repair_cands(nemo_ctx *c, uint32_t *out, uint64_t cap, uint64_t *n_out) {
  if (!c) return NEMO_ERR_INVALID;
  const std::vector<uint32_t> &cand = c->cs.rp.h_cand;
  return fetch_result(c, c->cs.rp.done, "nemo_fetch_min_repair_cands", REPAIR_CALLS, cand.data(), cand.size(), 4, out, cap, n_out);
}

}  // extern "C"
