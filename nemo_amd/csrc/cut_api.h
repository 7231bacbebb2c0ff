// cut_api.h — the host code the two searches of sets of size <= 3 over one graph share (api_cuts.hip: nemo_min_cuts;
// api_repair.hip: nemo_min_repair_sets, nemo_min_repairs; DESIGN.md §Minimal cut sets, §Minimal repair sets): the
// entry checks and the search from "the candidates are on the device" to the rows (the fetches' copy is knock_api.h's
// fetch_result).  What a round launches, its tier rule and what round 1's words decide are the calling entry point's,
// passed in NodeSearch and two callables.  The storage is the calling entry point's (ctx.h: its CutBufs, pinned buffer
// and event, handed in); while a search runs the driver owns it: it grows every buffer of the CutBufs but cand, grows
// the pinned buffer and waits on the event.  The rounds' sizes and the rows are knock_api.h's; the arithmetic is
// cut_host.h's.
#pragma once
#include "knock_api.h"

// cond is 0 or 1
static inline int node_search_cond(nemo_ctx *c, const char *who, int cond) {
  if (cond != 0 && cond != 1) return fail(c, NEMO_ERR_INVALID, "%s: cond must be 0 (pre) or 1 (post)", who);
  return NEMO_OK;
}

// The checks every entry point of the two searches starts with; b.done is void from here on.  cond: checked here,
// before flags and max_size, if given (nemo_min_cuts); nemo_min_repair_sets checks its own behind them, as it always has.
static inline int node_search_begin(nemo_ctx *c, const char *who, CutBufs CorpusState::*b, const int *cond, uint32_t max_size, uint32_t flags) {
  if (c && c->node) return fail(c, NEMO_ERR_STATE, "%s: single-device contexts only (a node context does not fan it out)", who);
  if (!c) return NEMO_ERR_INVALID;
  if (!c->cs.loaded) return fail(c, NEMO_ERR_STATE, "%s without a loaded corpus (the last load failed?)", who);
  (c->cs.*b).done = false;
  if (cond)
    if (int rc = node_search_cond(c, who, *cond)) return rc;
  if (flags) return fail(c, NEMO_ERR_INVALID, "%s: unknown flags %#x", who, flags);
  if (max_size < 1 || max_size > CUT_MAX_SIZE) return fail(c, NEMO_ERR_INVALID, "%s: max_size must be 1, 2 or 3 (%u)", who, max_size);
  return NEMO_OK;
}

// a search without a decision of its own (nemo_min_cuts)
static inline bool node_search_goes_on(const uint64_t *, uint64_t, double, double, int *) { return false; }

struct NodeSearch {  // what differs between the calls, beside its launch and decide callables
  const char *who;
  uint32_t g;         // 2r + cond
  uint32_t max_size;
  bool (*lds_fits)(uint64_t V, uint64_t E, uint64_t L, uint32_t lds_max);  // the tier rule
  uint32_t (*lds_bytes)(uint32_t V, uint32_t E, uint32_t L);               // ... and the LDS tier's image
  uint32_t (*lds_resident)(uint32_t size, uint32_t lds_bytes, uint32_t n_cu);  // the resident workgroups of a round's LDS kernel
  const char *lds_name, *glob_name;  // the sweeps' timing names
  bool round0;         // a round 0 (one chunk of two hypotheses, S = {} and S = every candidate) runs before round 1;
                       // its word lies behind round 1's in w[0]
  double image_extra;  // bytes a workgroup reads beside the graph's image (the repairs' bitmap)
  bool cand_from_dev;  // b.h_cand is not known yet: the candidates come back with round 1's words
  uint64_t *stats;     // the nine round stats
};

// The search over graph ns.g with its K candidates in b.cand (queued on the stream) and L Kahn levels.  h / ev: the
// call's pinned buffer and event; bytes: what the call has moved so far.  Rounds 0 and 1 run back to back and their
// words come back in one copy (K / 8 bytes), from which the host compacts the live list and uploads it; rounds 2
// and 3 follow without a round trip; the rows are cut_rows'.  The call's own, as lin_levels takes its callables:
//   launch(a, lds, grid, lds_bytes)        round a.size's sweep on the tier
//   decide(words, ck1, bytes, ops, &rc)    once rounds 0 and 1's words are on the host (round 0's at words[ck1]): true
//                                          ends the call with rc, and the timing group is the hook's to end
template <class LA, class DE>
static int node_search(nemo_ctx *c, const NodeSearch &ns, CutBufs &b, Pinned<uint32_t> &h, hipEvent_t ev, uint64_t K, uint32_t L,
                       GroupTimer &timer, double bytes, LA &&launch, DE &&decide) {
  CorpusState &cs = c->cs;
  const char *who = ns.who;
  const uint32_t g = ns.g, max_size = ns.max_size;
  const uint64_t V = cs.nv(g), E = cs.ne(g);
  hipStream_t s = c->stream;
  int rc;
  double ops = 0;
  if (!cuts::round_fits(K, 1))
    return fail(c, NEMO_ERR_LIMIT, "%s: %llu hypotheses of size 1 exceed 2^32 - 2: shorten the candidate list", who, (unsigned long long)K);
  // the tier and the grid: as many workgroups as are resident, at most one per chunk
  const bool lds = ns.lds_fits(V, E, L, c->opt.knock_lds_max);
  const uint32_t lds_bytes = lds ? ns.lds_bytes((uint32_t)V, (uint32_t)E, L) : 0u;
  const uint64_t dw = knock::dead_words(V);
  uint64_t resident = cuts::glob_resident(cs.dc.n_cu, dw);  // the global tier's
  if (lds) {
    const uint32_t first = ns.round0 ? 0u : 1u;
    for (uint32_t sz = first; sz <= max_size; sz++) {  // the rounds' kernels: the fewest of them
      const uint32_t n = ns.lds_resident(sz, lds_bytes, cs.dc.n_cu);
      if (!n) return fail(c, NEMO_ERR_HIP, "%s: no workgroup of %s is resident at %u bytes of LDS", who, ns.lds_name, lds_bytes);
      resident = sz == first ? n : std::min<uint64_t>(resident, n);
    }
  }
  const uint64_t ck1 = cuts::chunks(K), w0 = cuts::first_words(K, ns.round0);
  {
    const uint64_t need[3] = {2 * K, w0, lds ? 1 : dw * cuts::grid(cuts::chunks(cuts::most_hyps(K, max_size)), resident, c->opt.cut_grid)};
    if ((rc = grow_group(c, need, b.live, b.w[0], b.dead))) return rc;
  }
  if ((rc = h.grow(c, cuts::first_pinned(K, ns.round0)))) return rc;
  // one round: the byte model is the image read once per workgroup (4 E + 12 V + 4 L + 8, and the call's extra), 8
  // bytes written per chunk and 4 read per seed (round 0: every candidate once); the global tier reads the image
  // and rewrites its 8 V dead words per chunk
  const double image = 4.0 * (double)E + 12.0 * (double)V + 4.0 * (double)L + 8.0 + ns.image_extra;
  auto sweep = [&](const nemo::CutArgs &a) -> int {
    if (!a.n_chunks) return NEMO_OK;
    const uint32_t grid = cuts::grid(a.n_chunks, resident, c->opt.cut_grid);
    const double seeds = a.size ? 4.0 * (double)a.size * (double)a.n_hyp : 4.0 * (double)K;
    const double bt = lds ? grid * image + 8.0 * a.n_chunks + seeds : a.n_chunks * (image + 16.0 * (double)V + 8.0) + seeds;
    const double o = (double)a.n_chunks * (double)E;
    bytes += bt, ops += o;
    return timed(c, lds ? ns.lds_name : ns.glob_name, bt, o, [&] { launch(a, lds, grid, lds_bytes); });
  };
  nemo::CutArgs a[3] = {};
  for (uint32_t k = 0; k < 3; k++) {
    a[k].graph = g, a[k].size = k + 1, a[k].cand = b.cand.p, a[k].dead = b.dead.p;
  }
  if (ns.round0) {  // one chunk, its word behind round 1's
    nemo::CutArgs a0 = a[0];
    a0.size = 0, a0.n_hyp = 2, a0.n_chunks = 1, a0.words = b.w[0].p + ck1;
    if ((rc = sweep(a0))) return rc;
  }
  // round 1: every candidate is live
  a[0].n_hyp = (uint32_t)K, a[0].n_chunks = (uint32_t)ck1, a[0].live = nullptr, a[0].lnode = b.cand.p;
  a[0].words = b.w[0].p;
  if ((rc = sweep(a[0]))) return rc;
  {
    nemo::HostCopies hc;
    hc.add(h.p, b.w[0].p, 8 * w0);
    if (ns.cand_from_dev) hc.add(h.p + 2 * w0, b.cand.p, 4 * K);
    nemo::launch_to_host_multi(hc, s);
    if ((rc = wait_copied(c, ev))) return rc;
  }
  if (ns.cand_from_dev) b.h_cand.assign(h.p + 2 * w0, h.p + 2 * w0 + K);
  const uint64_t *w1 = reinterpret_cast<const uint64_t *>(h.p);
  if (decide(w1, ck1, bytes, ops, &rc)) return rc;
  std::vector<uint32_t> live = cuts::live_list(w1, K);  // the candidates that are no cut / no repair alone
  const uint64_t K1 = live.size();
  CutRounds rd;
  if ((rc = cut_rounds(K, K1, max_size, [&](uint64_t k, uint32_t sz) -> int {
         if (cuts::round_fits(k, sz)) return NEMO_OK;
         return fail(c, NEMO_ERR_LIMIT, "%s: the sets of %u of %llu live candidates exceed 2^32 - 2 hypotheses: shorten the candidate list", who,
                     sz, (unsigned long long)k);
       }, &rd)))
    return rc;
  {
    const uint64_t need[3] = {rd.ck[1], rd.ck[2], rd.scan_need};
    if ((rc = grow_group(c, need, b.w[1], b.w[2], b.scan))) return rc;
  }
  if (max_size >= 2 && K1) {
    b.h_live.resize(2 * K1);
    for (uint64_t p = 0; p < K1; p++) {
      b.h_live[p] = live[p];
      b.h_live[K1 + p] = b.h_cand[live[p]];
    }
    HIPCHK(c, hipMemcpyAsync(b.live.p, b.h_live.data(), 2 * K1 * 4, hipMemcpyHostToDevice, s));
  }
  for (uint32_t k = 1; k < max_size; k++) {
    a[k].n_hyp = (uint32_t)rd.n_hyp[k], a[k].n_chunks = (uint32_t)rd.ck[k];
    a[k].live = b.live.p, a[k].lnode = b.live.p + K1;
    a[k].words = b.w[k].p, a[k].pairs = k == 2 ? b.w[1].p : nullptr;
    if ((rc = sweep(a[k]))) return rc;
  }
  const CutOut out = {h, ev, b.scan, b.rows, 4, ns.stats, &b.n_rows, &b.done};
  return cut_rows(c, out, rd, a, max_size, timer, bytes, ops);
}
