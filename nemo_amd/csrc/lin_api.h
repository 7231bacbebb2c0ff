// lin_api.h — the host code the lineage searches share (api_lineage.hip: nemo_lineage_cuts; api_lgcuts.hip:
// nemo_lineage_group_cuts; api_lrepair.hip: nemo_lineage_repair_sets, nemo_lineage_repairs; DESIGN.md §Lineage-driven
// cut search): the level loop of the hitting-set tree, with the rule by which a level runs again behind a grown
// emission buffer (lin_host.h's lin::level_end), and the found sets' way to the host; and, for the searches over one
// graph (the cuts and the repairs), the tail from the tier choice to the rows, lin_node_search.  What a level
// evaluates, its limits and its bound are the calling entry point's, passed as callables.  Every call keeps its own
// event, pinned buffer, LinBufs and state (ctx.h); nothing here owns any.
#pragma once
#include "knock_api.h"

// The levels 0 .. max_size of a search over K candidates.  who / shorten: the calling entry point's name and what its
// messages tell the caller to shorten.  b: the call's buffers, b.ctr in place; col: a [cuts] column that grows and is
// kept alongside b.cuts (the group search's lost counts), or null; h / ev: the call's pinned buffer (8 elements at
// least) and event.  `a` is the level as the kernels read it: the loop fills everything but graph, cand, lds_total,
// region and region_words, which are the caller's.  Per level, in this order:
//   level_limit(n_front, d)       the call's own check of the level (a frontier past 2^32 - 2 sets; the group search's
//                                 lost words), with its own message; 0 if it fits
//   prepare(d, n_front, chunks)   behind the growth of the cuts' list, before the first pass
//   evaluate(pass, &bytes, &ops)  queues the evaluation of `a` (pass 1: the level once more, its cuts in place)
//   emit_bound(n_front, d)        the most children the level can count
// A pass zeroes the two counters behind the cuts', evaluates, and if the level emits zeroes the children's table and
// queues k_lin_filter; it reads one block of three counters from pinned memory and lin::level_end decides.
// stats[2 d], stats[2 d + 1]: sets evaluated, cuts found.  *n_cuts: the cuts in b.cuts (and col) at the end.
template <class LL, class P, class E, class B>
static int lin_levels(nemo_ctx *c, const char *who, const char *shorten, LinBufs &b, Pinned<uint64_t> &h, hipEvent_t ev, nemo::LinArgs &a,
                      uint64_t K, uint32_t max_size, uint64_t *stats, DevBuf<uint32_t> *col, LL &&level_limit, P &&prepare, E &&evaluate,
                      B &&emit_bound, double *bytes, double *ops, uint64_t *n_cuts_out) {
  hipStream_t s = c->stream;
  int rc;
  // the emission buffer (it starts small), the frontier and the children's table; the cuts' list, column and table
  uint64_t kids_cap = std::max<uint64_t>(b.kids.cap / 2, LIN_EMIT_START);
  if ((rc = grow_drop(c, b.kids, 2 * kids_cap)) || (rc = grow_drop(c, b.ktab, lin::table_slots(kids_cap))) ||
      (rc = grow_drop(c, b.front, 2 * kids_cap)))
    return rc;
  uint64_t cuts_cap = std::max<uint64_t>(col ? std::min(b.cuts.cap / 2, col->cap) : b.cuts.cap / 2, LIN_MIN_TABLE);
  if ((rc = grow_drop(c, b.cuts, 2 * cuts_cap)) || (col && (rc = grow_drop(c, *col, cuts_cap))) ||
      (rc = grow_drop(c, b.ctab, lin::table_slots(cuts_cap))))
    return rc;
  uint64_t cslots = lin::table_slots(cuts_cap);
  nemo::launch_zero(b.ctab.p, 4 * cslots, s);
  nemo::launch_zero(b.ctr.p, 32, s);
  {  // level 0's frontier: the empty set, every field LIN_PAD
    static const uint64_t empty[2] = {~0ull, ~0ull};
    HIPCHK(c, hipMemcpyAsync(b.front.p, empty, 16, hipMemcpyHostToDevice, s));
  }
  a.K = (uint32_t)K, a.ctr = b.ctr.p;
  uint64_t n_front = 1, n_cuts = 0;
  uint32_t cut_sizes = 0;
  volatile const uint64_t *hctr = h.p;
  for (uint32_t d = 0; d <= max_size; d++) {
    if ((rc = level_limit(n_front, d))) return rc;
    stats[2 * d] = n_front;
    const uint64_t grown = lin::cuts_grown(cuts_cap, n_cuts, n_front);
    if (grown != cuts_cap) {  // every set of the level may be a cut: the list and the column with their contents, the table anew
      if ((rc = grow_keep(c, b.cuts, 2 * grown, 2 * n_cuts)) || (col && (rc = grow_keep(c, *col, grown, n_cuts))) ||
          (rc = grow_drop(c, b.ctab, lin::table_slots(grown))))
        return rc;
      cuts_cap = grown, cslots = lin::table_slots(grown);
      nemo::launch_zero(b.ctab.p, 4 * cslots, s);
      a.cuts = b.cuts.p, a.ctab = b.ctab.p, a.cslots = cslots;
      if ((rc = timed(c, "k_lin_rehash", 20.0 * (double)n_cuts, 0, [&] { nemo::launch_lin_rehash(a, n_cuts, s); }))) return rc;
    }
    const bool emit = d < max_size;
    const uint64_t ck = lin::chunks(n_front);
    if ((rc = prepare(d, n_front, ck))) return rc;
    for (int pass = 0;; pass++) {
      nemo::launch_zero(b.ctr.p + 1, 16, s);
      a.front = b.front.p, a.n_front = (uint32_t)n_front, a.n_chunks = (uint32_t)ck;
      a.emit = emit ? 1u : 0u, a.redo = pass ? 1u : 0u;
      a.kids = b.kids.p, a.kids_cap = kids_cap;
      a.cuts = b.cuts.p, a.ctab = b.ctab.p, a.cslots = cslots;
      a.next = b.front.p, a.cut_sizes = cut_sizes, a.size = d, a.cuts_before = n_cuts;
      if ((rc = evaluate(pass, bytes, ops))) return rc;
      if (emit) {
        const uint64_t most = std::min<uint64_t>(kids_cap, emit_bound(n_front, d));
        a.ktab = b.ktab.p, a.kslots = lin::table_slots(most);
        nemo::launch_zero(b.ktab.p, 4 * a.kslots, s);
        const double bf = 4.0 * (double)a.kslots;
        if ((rc = timed(c, "k_lin_filter", bf, 0, [&] { nemo::launch_lin_filter(a, lin::filter_grid(most, LIN_BLOCK, 8ull * c->cs.dc.n_cu), s); })))
          return rc;
        *bytes += bf;
      }
      nemo::launch_to_host(h.p, b.ctr.p, 32, s);
      if ((rc = wait_copied(c, ev))) return rc;
      const uint64_t counted = hctr[1];
      const lin::LevelEnd end = emit ? lin::level_end(counted, kids_cap, c->opt.lin_children_max, pass) : lin::LEVEL_DONE;
      if (end == lin::LEVEL_DONE) break;
      if (end == lin::LEVEL_LIMIT)
        return fail(c, NEMO_ERR_LIMIT,
                    "%s: level %u emits %llu children, more than the option \"lineage_children_max\" allows (%llu): raise it, or shorten the %s", who,
                    d, (unsigned long long)counted, (unsigned long long)c->opt.lin_children_max, shorten);
      if (end == lin::LEVEL_BROKEN)
        return fail(c, NEMO_ERR_HIP, "%s: level %u counted %llu children behind a buffer grown to its first count", who, d,
                    (unsigned long long)counted);
      // the level overflowed: the buffer to the counted size, the frontier kept, and the level once more
      kids_cap = lin::emit_grown(kids_cap, counted);
      if ((rc = grow_drop(c, b.kids, 2 * kids_cap)) || (rc = grow_drop(c, b.ktab, lin::table_slots(kids_cap))) ||
          (rc = grow_keep(c, b.front, 2 * kids_cap, 2 * n_front)))
        return rc;
    }
    const uint64_t cuts_now = hctr[0];
    stats[2 * d + 1] = cuts_now - n_cuts;
    if (cuts_now > n_cuts) cut_sizes |= 1u << d;
    n_cuts = cuts_now;
    if (!emit) break;
    n_front = hctr[2];
    if (!n_front) break;
  }
  *n_cuts_out = n_cuts;
  return NEMO_OK;
}

struct LinCuts {
  std::vector<lin::Key> keys;        // [n_cuts] as the device holds them
  std::vector<uint32_t> col;         // ... and the column's entries, if there is one
  std::vector<uint32_t> order;       // the rows' order: row i is keys[order[i]]
};

// The n_cuts keys of b.cuts (and the entries of col, if given) through the call's pinned buffer, and the order of the
// rows: (size, colex), lin::row_less.
static inline int lin_sorted_keys(nemo_ctx *c, const LinBufs &b, const DevBuf<uint32_t> *col, Pinned<uint64_t> &h, hipEvent_t ev,
                                  uint64_t n_cuts, LinCuts *out) {
  out->keys.resize(n_cuts), out->order.resize(n_cuts), out->col.resize(col ? n_cuts : 0);
  if (!n_cuts) return NEMO_OK;
  int rc;
  if ((rc = h.grow(c, 2 * n_cuts + (col ? n_cuts / 2 + 1 : 0)))) return rc;
  nemo::launch_to_host(h.p, b.cuts.p, 16 * n_cuts, c->stream);
  if (col) nemo::launch_to_host(h.p + 2 * n_cuts, col->p, 4 * n_cuts, c->stream);
  if ((rc = wait_copied(c, ev))) return rc;
  const uint32_t *hn = reinterpret_cast<const uint32_t *>(h.p + 2 * n_cuts);
  for (uint64_t i = 0; i < n_cuts; i++) {
    out->keys[i] = lin::Key{h.p[2 * i], h.p[2 * i + 1]}, out->order[i] = (uint32_t)i;
    if (col) out->col[i] = hn[i];
  }
  std::sort(out->order.begin(), out->order.end(), [&](uint32_t x, uint32_t y) { return lin::row_less(out->keys[x], out->keys[y]); });
  return NEMO_OK;
}

struct LinSearch {  // what differs between the two lineage searches over one graph, beside their launch and before callables
  const char *who;
  uint32_t g;         // 2r + cond
  uint32_t max_size;
  bool (*lds_fits)(uint64_t V, uint64_t E, uint64_t L, uint32_t lds_max);  // the tier rule (option wit_lds_max)
  uint32_t (*lds_bytes)(uint32_t V, uint32_t E, uint32_t L);               // ... and the LDS tier's image
  uint64_t (*glob_words)(uint64_t V);                      // a workgroup's region on the global tier, in u64
  double (*image_bytes)(double V, double E, double L);     // the bytes a workgroup reads to stage the graph
  uint32_t (*lds_resident)(uint32_t lds_bytes, uint32_t n_cu);  // the resident workgroups of the LDS-tier kernel
  const char *lds_name, *glob_name;  // the evaluations' timing names
  double glob_node_bytes;  // the global tier's bytes per node per chunk: 16 per word array of the region
  uint64_t *stats;         // [18] per size 0..8: sets evaluated, sets found
};

// a search with nothing to do before the levels (nemo_lineage_cuts)
static inline bool lin_search_goes_on(const nemo::LinArgs &, bool, double *, double *, int *) { return false; }

// The rows of both searches are {size, node[8]}: one layout, filled by one loop.
static_assert(sizeof(nemo_lineage_cut) == sizeof(nemo_lineage_repair) && offsetof(nemo_lineage_cut, node) == offsetof(nemo_lineage_repair, node),
              "nemo_lineage_cut and nemo_lineage_repair share one layout");

// The search over graph ls.g with its candidates h_cand in d_cand (queued on the stream) and L Kahn levels, from the
// tier choice to the rows: the tier and the launch's LDS, the grid (as many workgroups as are resident, at most one
// per chunk), the growth of b.ctr and the workgroups' region together, the level loop, and the found sets as rows
// sorted by (size, colex), their positions turned into nodes through h_cand.  h / ev: the call's pinned buffer (8
// elements at least) and event; bytes: what the call has moved so far.  The call's own, as node_search takes its
// callables:
//   launch(a, lds, grid)                  the evaluation of level `a` on the tier
//   before(a, lds, &bytes, &ops, &rc)     once the buffers are grown and `a` names them, before the levels (the
//                                         repairs' two-hypothesis launch): true ends the call with rc, and the timing
//                                         group is the hook's to end
// The byte model of a level: a workgroup reads the image once; a set is 16 bytes read; the global tier adds
// ls.glob_node_bytes V per chunk for its word arrays; the children are not known at the launch and are left out;
// ops = 2 E child words per chunk, one sweep up and one pass down.  Ends the call's timing group behind the levels.
template <class Row, class LA, class BE>
static int lin_node_search(nemo_ctx *c, const LinSearch &ls, LinBufs &b, DevBuf<uint64_t> &region, const DevBuf<uint32_t> &d_cand,
                           const std::vector<uint32_t> &h_cand, Pinned<uint64_t> &h, hipEvent_t ev, uint32_t L, GroupTimer &timer, double bytes,
                           std::vector<Row> *rows, LA &&launch, BE &&before) {
  CorpusState &cs = c->cs;
  const char *who = ls.who;
  const uint64_t V = cs.nv(ls.g), E = cs.ne(ls.g), K = h_cand.size();
  int rc;
  double ops = 0;
  const bool lds = ls.lds_fits(V, E, L, c->opt.wit_lds_max);
  const uint32_t image = lds ? ls.lds_bytes((uint32_t)V, (uint32_t)E, L) : 0u;
  const uint64_t rw = lds ? 0 : ls.glob_words(V);
  uint32_t lds_total = 0, res_lds = 1;
  if (lds && (rc = ko_lds_total(c, who, ls.lds_name, [&](uint32_t by) { return ls.lds_resident(by, cs.dc.n_cu); }, image, 0, 4096, &lds_total,
                                &res_lds)))
    return rc;
  const uint32_t cap = c->opt.kl_grid;
  const uint64_t resident = lds ? res_lds : klabel::region_grid(2ull * cs.dc.n_cu, rw);
  {
    const uint64_t need[2] = {4, std::max<uint64_t>(1, rw * lin::grid(~0ull, resident, cap))};
    if ((rc = grow_group(c, need, b.ctr, region))) return rc;
  }
  nemo::LinArgs a{};
  a.graph = ls.g, a.cand = d_cand.p, a.K = (uint32_t)K, a.ctr = b.ctr.p;
  a.lds_total = lds_total, a.region = region.p, a.region_words = rw;
  if (before(a, lds, &bytes, &ops, &rc)) return rc;
  const double img = ls.image_bytes((double)V, (double)E, (double)L);
  auto level_limit = [&](uint64_t n_front, uint32_t d) -> int {
    if (lin::front_fits(n_front)) return NEMO_OK;
    return fail(c, NEMO_ERR_LIMIT, "%s: a frontier of %llu sets of size %u exceeds 2^32 - 2: shorten the candidate list", who,
                (unsigned long long)n_front, d);
  };
  auto prepare = [](uint32_t, uint64_t, uint64_t) { return NEMO_OK; };  // nothing is sized by the level
  auto evaluate = [&](int, double *by, double *op) -> int {
    const uint64_t ck = a.n_chunks;
    const uint32_t grid = lin::grid(ck, resident, cap);
    const double bt = grid * img + 16.0 * (double)a.n_front + (lds ? 0.0 : (double)ck * ls.glob_node_bytes * (double)V);
    const double o = (double)ck * 2.0 * (double)E;
    *by += bt, *op += o;
    return timed(c, lds ? ls.lds_name : ls.glob_name, bt, o, [&] { launch(a, lds, grid); });
  };
  auto emit_bound = [&](uint64_t n_front, uint32_t d) { return lin::emit_bound(n_front, K, d); };
  uint64_t n_found = 0;
  if ((rc = lin_levels(c, who, "candidate list", b, h, ev, a, K, ls.max_size, ls.stats, nullptr, level_limit, prepare, evaluate, emit_bound,
                       &bytes, &ops, &n_found)))
    return rc;
  timer.done(bytes, ops);
  LinCuts found;
  if ((rc = lin_sorted_keys(c, b, nullptr, h, ev, n_found, &found))) return rc;
  rows->resize(n_found);
  for (uint64_t i = 0; i < n_found; i++) {
    Row &row = (*rows)[i];
    uint32_t pos[LIN_MAX_SIZE];
    row.size = lin::key_unpack(found.keys[found.order[i]], pos);
    for (uint32_t j = 0; j < LIN_MAX_SIZE; j++) row.node[j] = j < row.size ? h_cand[pos[j]] : 0xFFFFFFFFu;
  }
  return NEMO_OK;
}
