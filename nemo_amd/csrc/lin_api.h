// lin_api.h — the host code the two lineage searches share (api_lineage.hip: nemo_lineage_cuts; api_lgcuts.hip:
// nemo_lineage_group_cuts; DESIGN.md §Lineage-driven cut search): the level loop of the hitting-set tree, with the
// rule by which a level runs again behind a grown emission buffer (lin_host.h's lin::level_end), and the cuts' way to
// the host.  What a level evaluates, its limits and its bound are the calling entry point's, passed as callables.
// Every call keeps its own event, pinned buffer, LinBufs and state (ctx.h); nothing here owns any.
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
