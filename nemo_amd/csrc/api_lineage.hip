// api_lineage.hip — nemo_lineage_cuts and its fetches (k_lineage.hip, lin_host.h; DESIGN.md §Lineage-driven cut
// search).  The level counts, the wait for the copies, the buffer group and the timing group are knock_api.h's and
// ctx.h's, shared with the knock-out family; the tier rule and image are the witness calls' (wit_host.h).  The call
// keeps its entry checks, its early ends and its candidate source (the caller's list, or the sink goals k_ko_leaves
// lists); the search from there to the rows is lin_api.h's lin_node_search, shared with api_lrepair.hip: the host
// drives the levels (lin_levels, shared with nemo_lineage_group_cuts too), per level it queues the evaluation and the
// filter, reads one block of three counters from pinned memory, and decides whether the level runs again behind a
// grown emission buffer.
#include "knock_api.h"
#include "lin_api.h"

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
  const uint64_t V = cs.nv(g);
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
  double bytes = 0;
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
  {  // the candidates on the device
    const uint64_t need = std::max<uint64_t>(K, 1);
    if ((rc = grow_group(c, &need, cs.d_lncand))) return rc;
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
  LinSearch ls{who, g, max_size, wit::lds_fits, wit::wit_lds_bytes, wit::glob_words, wit::image_bytes, nemo::lin_lds_resident, "k_lin_lds",
               "k_lin_glob"};
  ls.glob_node_bytes = 32.0, ls.stats = cs.lin_stats;  // the dead and the need words
  auto launch = [&](const nemo::LinArgs &a, bool lds, uint32_t grid) {
    if (lds) nemo::launch_lin_lds(cs.dc, a, grid, s);
    else nemo::launch_lin_glob(cs.dc, a, grid, s);
  };
  if ((rc = lin_node_search(c, ls, cs.d_ln, cs.d_lnreg, cs.d_lncand, cs.lin_cand, c->h_lin, c->ev_lin, L, timer, bytes, &cs.lin_rows, launch,
                            lin_search_goes_on)))
    return rc;
  cs.lin_done = true;
  return NEMO_OK;
}

int nemo_fetch_lineage_cuts(nemo_ctx *c, nemo_lineage_cut *out, uint64_t cap, uint64_t *n_out) {
  if (!c) return NEMO_ERR_INVALID;
  const std::vector<nemo_lineage_cut> &rows = c->cs.lin_rows;
  return fetch_result(c, c->cs.lin_done, "nemo_fetch_lineage_cuts", "nemo_lineage_cuts", rows.data(), rows.size(), sizeof(nemo_lineage_cut), out, cap,
                      n_out);
}

int nemo_fetch_lineage_cut_stats(nemo_ctx *c, uint64_t out[18]) {
  if (!c || !out) return NEMO_ERR_INVALID;
  return fetch_result(c, c->cs.lin_done, "nemo_fetch_lineage_cut_stats", "nemo_lineage_cuts", c->cs.lin_stats, 18, 8, out, 18, nullptr);
}

}  // extern "C"
