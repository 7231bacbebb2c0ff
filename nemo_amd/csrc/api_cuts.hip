// api_cuts.hip — nemo_min_cuts and its fetches (k_cuts.hip, cut_host.h; DESIGN.md §Minimal cut sets).  The call
// keeps its entry checks and its candidate source; the search from there to the rows is cut_api.h's node_search,
// shared with api_repair.hip.
#include "cut_api.h"

extern "C" {

// Rounds of sizes 1, 2, 3 over the sink goals (k_ko_leaves counts and lists them) or the caller's candidates.
int nemo_min_cuts(nemo_ctx *c, uint32_t iteration, int cond, const uint32_t *cand, size_t n_cand, uint32_t max_size,
                  uint32_t flags) {
  const char *who = "nemo_min_cuts";
  int rc;
  if ((rc = node_search_begin(c, who, &CorpusState::cut, &cond, max_size, flags))) return rc;
  CorpusState &cs = c->cs;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_whole(c))) return rc;  // reads the graph's build outputs
  if ((rc = ensure_load_checked(c))) return rc;
  uint32_t r;
  if ((rc = run_index(c, iteration, &r))) return rc;
  const uint32_t g = 2 * r + (uint32_t)cond;
  const uint64_t V = cs.nv(g);
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
  cs.cut.n_rows = 0;
  if (cand && n_cand == 0) {  // zero hypotheses
    cs.cut.done = true;
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
  double bytes = 0;
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
    cs.cut.done = true;
    return NEMO_OK;
  }
  // the candidates on the device
  if ((rc = grow_group(c, &K, cs.cut.cand))) return rc;
  if (cand) {
    cs.cut.h_cand.assign(cand, cand + K);
    HIPCHK(c, hipMemcpyAsync(cs.cut.cand.p, cs.cut.h_cand.data(), K * 4, hipMemcpyHostToDevice, s));
  } else {
    cs.cut_up[2] = 0u, cs.cut_up[3] = (uint32_t)K;
    HIPCHK(c, hipMemcpyAsync(desc + 1, cs.cut_up + 2, 8, hipMemcpyHostToDevice, s));
    ka.leaf = cs.cut.cand.p;
    const double b_leaves = 8.0 * (double)V + 12.0 + 4.0 * (double)K;
    if ((rc = timed(c, "k_ko_leaves", b_leaves, 0, [&] { nemo::launch_ko_leaves(cs.dc, ka, true, s); }))) return rc;
    bytes += b_leaves;
  }
  NodeSearch ns{who, g, max_size, knock::lds_fits, knock::knock_lds_bytes, nemo::cut_lds_resident, "k_cut_lds", "k_cut_glob"};
  ns.round0 = false, ns.image_extra = 0, ns.cand_from_dev = !cand, ns.stats = cs.cut_stats;
  auto launch = [&](const nemo::CutArgs &a, bool lds, uint32_t grid, uint32_t lds_bytes) {
    if (lds) nemo::launch_cut_lds(cs.dc, a, grid, lds_bytes, s);
    else nemo::launch_cut_glob(cs.dc, a, grid, s);
  };
  return node_search(c, ns, cs.cut, c->h_cuts, c->ev_cuts, K, L, timer, bytes, launch, node_search_goes_on);
}

int nemo_fetch_min_cuts(nemo_ctx *c, nemo_cut *out, uint64_t cap, uint64_t *n_out) {
  if (!c) return NEMO_ERR_INVALID;
  return fetch_result(c, c->cs.cut.done, "nemo_fetch_min_cuts", "nemo_min_cuts", c->h_cuts.p, c->cs.cut.n_rows, sizeof(nemo_cut), out, cap, n_out);
}

int nemo_fetch_min_cut_stats(nemo_ctx *c, uint64_t out[9]) {
  if (!c || !out) return NEMO_ERR_INVALID;
  return fetch_result(c, c->cs.cut.done, "nemo_fetch_min_cut_stats", "nemo_min_cuts", c->cs.cut_stats, 9, 8, out, 9, nullptr);
}

}  // extern "C"
