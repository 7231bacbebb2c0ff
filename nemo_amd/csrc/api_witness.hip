// api_witness.hip — nemo_witness_sets, nemo_witness_labels and their fetches (k_witness.hip, wit_host.h; DESIGN.md
// §Surviving derivations).  The level counts, the tier split, the launch's dynamic LDS, the wait for the copies, the
// buffer group and the timing group are knock_api.h's and ctx.h's, shared with the knock-out family.
#include "knock_api.h"

namespace {

// what both entry points check first; leaves the device set and the graphs whole
int wit_enter(nemo_ctx *c, const char *who, int cond, uint32_t flags, uint32_t known) {
  CorpusState &cs = c->cs;
  if (!cs.loaded) return fail(c, NEMO_ERR_STATE, "%s without a loaded corpus (the last load failed?)", who);
  cs.wit_done = false;
  cs.wit_masks = false;
  if (cond != 0 && cond != 1) return fail(c, NEMO_ERR_INVALID, "%s: cond must be 0 (pre) or 1 (post)", who);
  if (flags & ~known) return fail(c, NEMO_ERR_INVALID, "%s: unknown flags %#x", who, flags);
  return NEMO_OK;
}

// The call whose graphs (cs.wit_desc[0 .. n)), set offsets (cs.wit_setoff) and entries (cs.wit_ent: n_ent nodes, or
// n_ent rows and then the k1 distinct labels) are in place: the tiers, the buffers, the uploads, the two sweeps, the
// rows to pinned memory and the wait for them.
int wit_run(nemo_ctx *c, const char *who, size_t n, size_t n_sets, const uint32_t *ent, uint64_t n_ent, uint32_t k1, uint32_t flags) {
  CorpusState &cs = c->cs;
  std::vector<uint32_t> &desc = cs.wit_desc;
  const uint64_t ck = klabel::chunks(n_sets), hyps = (uint64_t)n * n_sets;
  int rc;
  if ((rc = ensure_event(c, &c->ev_wit))) return rc;
  hipStream_t s = c->stream;
  if ((rc = ensure_nlev(c, c->h_wit, c->ev_wit))) return rc;
  GroupTimer timer(c, "k_witness");
  const uint32_t lds_max = c->opt.wit_lds_max;
  auto fits = [&](uint32_t g) { return wit::lds_fits(cs.nv(g), cs.ne(g), cs.kl_nlev[g], lds_max); };
  auto image = [&](uint32_t g) { return wit::wit_lds_bytes((uint32_t)cs.nv(g), (uint32_t)cs.ne(g), cs.kl_nlev[g]); };
  const Tiers tr = split_tiers_by(c, desc, n, fits, image);
  if (k1 && lcuts::list_entries(k1, std::max(tr.lds_v, tr.glob_v)) > 0xFFFFFFFFull)
    return fail(c, NEMO_ERR_LIMIT, "%s: %u distinct labels and a graph of %llu nodes exceed a hit list of 2^32 - 1 entries: tile the call", who,
                k1, (unsigned long long)std::max(tr.lds_v, tr.glob_v));
  // the kept need words
  std::vector<uint64_t> v(n);
  for (size_t i = 0; i < n; i++) v[i] = cs.nv(desc[i]);
  uint64_t kept = 0;
  cs.wit_moff.assign(n, 0);
  if ((flags & NEMO_WIT_MASKS) && !wit::need_offsets(v.data(), n, ck, &cs.wit_moff, &kept))
    return fail(c, NEMO_ERR_LIMIT,
                "%s: the need words of %zu list positions x %llu chunks (8 bytes per node and chunk of 64 hypotheses) exceed 2^36 bytes: tile the call",
                who, n, (unsigned long long)ck);
  // the launch's LDS and what a workgroup keeps in device memory
  uint32_t lds_total = 0, res_lds = 1;
  uint64_t rw_lds = 0;
  if (tr.n_lds) {
    if ((rc = ko_lds_total(c, who, "k_wit_lds", [&](uint32_t b) { return nemo::wit_lds_resident(b, cs.dc.n_cu); }, tr.image,
                           k1 ? 4 * lcuts::list_entries(k1, tr.lds_v) : 0, 4096, &lds_total, &res_lds)))
      return rc;
    for (size_t k = 0; k < tr.n_lds; k++) {
      const uint32_t g = desc[desc[n + k]];
      rw_lds = std::max(rw_lds, wit::region_words(0, k1, cs.nv(g), (lds_total - image(g)) / 4u));
    }
  }
  const uint64_t glob_words = wit::glob_words(tr.glob_v);
  const uint64_t rw_glob = wit::region_words(glob_words, k1, tr.glob_v, 0);
  const uint32_t cap = c->opt.kl_grid;
  uint64_t r_lds = klabel::region_grid(res_lds, rw_lds), r_glob = klabel::region_grid(2ull * cs.dc.n_cu, rw_glob);
  if (cap) r_lds = std::min<uint64_t>(r_lds, cap), r_glob = std::min<uint64_t>(r_glob, cap);
  const klabel::Split sp_lds = klabel::split(tr.n_lds, ck, r_lds), sp_glob = klabel::split(tr.n_glob, ck, r_glob);
  const uint32_t grid_lds = klabel::grid(sp_lds.items, r_lds, cap), grid_glob = klabel::grid(sp_glob.items, r_glob, cap);
  const uint64_t slots = k1 ? klabel::table_slots(k1) : 1;
  {
    const uint64_t need[9] = {n_sets + 1, std::max<uint64_t>(n_ent + k1, 1), slots, slots, 2 * (uint64_t)n, (uint64_t)n, 5 * hyps, std::max<uint64_t>(kept, 1),
                              std::max<uint64_t>(1, std::max<uint64_t>(tr.n_lds ? grid_lds * rw_lds : 0ull, tr.n_glob ? grid_glob * rw_glob : 0ull))};
    if ((rc = grow_group(c, need, cs.d_wtset, cs.d_wtent, cs.d_wtkey, cs.d_wtval, cs.d_wtdesc, cs.d_wtmoff, cs.d_wtrows, cs.d_wtneed, cs.d_wtreg)))
      return rc;
  }
  if ((rc = c->h_wit.grow(c, 5 * hyps))) return rc;
  HIPCHK(c, hipMemcpyAsync(cs.d_wtset.p, cs.wit_setoff.data(), (n_sets + 1) * 8, hipMemcpyHostToDevice, s));
  if (n_ent + k1)  // (the call ends behind a wait for the stream: the caller's array outlives the copy)
    HIPCHK(c, hipMemcpyAsync(cs.d_wtent.p, ent, (n_ent + k1) * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(cs.d_wtdesc.p, desc.data(), 2 * n * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(cs.d_wtmoff.p, cs.wit_moff.data(), n * 8, hipMemcpyHostToDevice, s));
  nemo::WitArgs a{};
  a.set_off = cs.d_wtset.p, a.ent = cs.d_wtent.p, a.n_sets = (uint32_t)n_sets, a.n_chunks = (uint32_t)ck;
  a.k1 = k1, a.dist = cs.d_wtent.p + n_ent, a.key = cs.d_wtkey.p, a.val = cs.d_wtval.p, a.slots = slots;
  a.graph = cs.d_wtdesc.p;
  a.sinks = (flags & NEMO_WIT_SINKS) ? 1u : 0u, a.all = (flags & NEMO_WIT_ALL) ? 1u : 0u;
  a.region = cs.d_wtreg.p, a.rows = cs.d_wtrows.p;
  a.need = (flags & NEMO_WIT_MASKS) ? cs.d_wtneed.p : nullptr, a.moff = cs.d_wtmoff.p;
  double bytes = 8.0 * (double)(n_sets + 1) + 4.0 * (double)n_ent, ops = 0;
  if (k1) {
    nemo::launch_zero(cs.d_wtkey.p, 4 * slots, s);
    const double b_tab = 4.0 * (double)slots + 16.0 * (double)k1;
    if ((rc = timed(c, "k_wit_table", b_tab, 0, [&] { nemo::launch_wit_table(a, s); }))) return rc;
    bytes += b_tab;
  }
  // the byte model: a work item reads its graph's image (k_ko_lds's: 4 E + 12 V + 4 L + 8) and, in the label form,
  // 4 V labels twice; a chunk reads its sets' offsets and entries, writes 20 bytes per row and, where the need words
  // are kept, 8 V; the global tier adds 32 V per chunk for its two word arrays in device memory (each written and
  // read); ops = 2 E child words per chunk, one sweep up and one pass down
  for (int tier = 0; tier < 2; tier++) {
    const uint32_t nt = tier ? tr.n_glob : tr.n_lds;
    if (!nt) continue;
    const klabel::Split &sp = tier ? sp_glob : sp_lds;
    double b = 0, o = 0;
    for (uint32_t k = 0; k < nt; k++) {
      const uint32_t g = desc[desc[n + (tier ? tr.n_lds : 0) + k]];
      const double V = (double)cs.nv(g), E = (double)cs.ne(g), L = (double)cs.kl_nlev[g];
      b += sp.parts * (wit::image_bytes(V, E, L) + (k1 ? 8.0 * V : 0.0)) + 20.0 * (double)n_sets + 8.0 * (double)(n_sets + 1) +
           4.0 * (double)n_ent + (double)ck * (((flags & NEMO_WIT_MASKS) ? 8.0 * V : 0.0) + (tier ? 32.0 * V : 0.0));
      o += (double)ck * 2.0 * E;
    }
    a.pos = cs.d_wtdesc.p + n + (tier ? tr.n_lds : 0);
    a.n_tier = nt, a.parts = sp.parts;
    a.lds_total = tier ? 0u : lds_total;
    a.region_words = tier ? rw_glob : rw_lds;
    a.glob_words = tier ? glob_words : 0;
    if (tier) rc = timed(c, "k_wit_glob", b, o, [&] { nemo::launch_wit_glob(cs.dc, a, grid_glob, s); });
    else rc = timed(c, "k_wit_lds", b, o, [&] { nemo::launch_wit_lds(cs.dc, a, grid_lds, s); });
    if (rc) return rc;
    bytes += b, ops += o;
  }
  timer.done(bytes, ops);
  nemo::launch_to_host(c->h_wit.p, cs.d_wtrows.p, 20 * hyps, s);  // the rows to pinned memory
  if ((rc = wait_copied(c, c->ev_wit))) return rc;
  cs.wit_masks = (flags & NEMO_WIT_MASKS) != 0;
  cs.wit_done = true;
  return NEMO_OK;
}

}  // namespace

extern "C" {

// Explicit node sets on one graph: nemo_knockout_sets' arguments, checks and limits.
int nemo_witness_sets(nemo_ctx *c, uint32_t iteration, int cond, const uint64_t *set_off, const uint32_t *set_nodes, size_t n_sets,
                      uint32_t flags) {
  if (c && c->node)
    return fail(c, NEMO_ERR_STATE, "nemo_witness_sets: single-device contexts only (a node context does not fan it out)");
  if (!c || (!set_off && n_sets)) return NEMO_ERR_INVALID;
  CorpusState &cs = c->cs;
  int rc;
  if ((rc = wit_enter(c, "nemo_witness_sets", cond, flags, NEMO_WIT_ALL | NEMO_WIT_MASKS))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_whole(c))) return rc;  // may read any graph's build outputs
  if ((rc = ensure_load_checked(c))) return rc;
  uint32_t r;
  if ((rc = run_index(c, iteration, &r))) return rc;
  const uint32_t g = 2 * r + (uint32_t)cond;
  const uint64_t V = cs.nv(g);
  if (n_sets && set_off[n_sets] > set_off[0] && !set_nodes) return NEMO_ERR_INVALID;
  uint64_t where = 0;
  switch (knock::check_sets(set_off, set_nodes, n_sets, V, &where)) {
    case knock::SET_NONMONOTONE:
      return fail(c, NEMO_ERR_INVALID, "nemo_witness_sets: set_off decreases at set %llu", (unsigned long long)where);
    case knock::SET_NODE:
      return fail(c, NEMO_ERR_INVALID, "nemo_witness_sets: node %u at position %llu is out of range (%llu nodes)", set_nodes[where],
                  (unsigned long long)where, (unsigned long long)V);
    case knock::SET_LIMIT:
      return fail(c, NEMO_ERR_LIMIT, "nemo_witness_sets: the sets name more than 2^32 - 1 nodes: tile the call");
    default:
      break;
  }
  cs.wit_n = 1, cs.wit_sets = n_sets, cs.wit_chunks = klabel::chunks(n_sets);
  cs.wit_desc.assign(2, g);
  if (n_sets == 0) {  // zero hypotheses
    cs.wit_done = true;
    return NEMO_OK;
  }
  if (n_sets > KO_MAX_HYPS)
    return fail(c, NEMO_ERR_LIMIT, "nemo_witness_sets: %llu hypotheses exceed 2^32 - 2 in one call: tile the call", (unsigned long long)n_sets);
  std::vector<uint64_t> &off = cs.wit_setoff;  // relative to the first set
  off.resize(n_sets + 1);
  for (size_t k = 0; k <= n_sets; k++) off[k] = set_off[k] - set_off[0];
  cs.wit_ent.clear();
  return wit_run(c, "nemo_witness_sets", 1, n_sets, set_nodes ? set_nodes + set_off[0] : nullptr, off[n_sets], 0, flags);
}

// Label sets against every listed run: nemo_knockout_labels' arguments and checks.  The host sorts the distinct
// labels the sets name and rewrites the sets as rows of them; k_wit_table hashes label -> row.
int nemo_witness_labels(nemo_ctx *c, const uint32_t *iters, size_t n, int cond, const uint64_t *set_off, const uint32_t *set_labels,
                        size_t n_sets, uint32_t flags) {
  if (c && c->node)
    return fail(c, NEMO_ERR_STATE, "nemo_witness_labels: single-device contexts only (a node context does not fan it out)");
  if (!c || (!iters && n) || (!set_off && n_sets)) return NEMO_ERR_INVALID;
  CorpusState &cs = c->cs;
  int rc;
  if ((rc = wit_enter(c, "nemo_witness_labels", cond, flags, NEMO_WIT_ALL | NEMO_WIT_MASKS | NEMO_WIT_SINKS))) return rc;
  if (!klabel::sets_fit(n_sets))  // before set_off is read
    return fail(c, NEMO_ERR_LIMIT, "nemo_witness_labels: %zu sets exceed 2^32 - 1 in one call: tile the call", n_sets);
  uint64_t where = 0;
  switch (klabel::check_offsets(set_off, n_sets, &where)) {  // before any label is read
    case klabel::SET_NONMONOTONE:
      return fail(c, NEMO_ERR_INVALID, "nemo_witness_labels: set_off decreases at set %llu", (unsigned long long)where);
    case klabel::SET_LIMIT:
      return fail(c, NEMO_ERR_LIMIT, "nemo_witness_labels: the sets name more than 2^32 - 1 labels: tile the call");
    default:
      break;
  }
  const uint64_t n_labels = n_sets ? set_off[n_sets] - set_off[0] : 0;
  if (n_labels && !set_labels) return NEMO_ERR_INVALID;
  if (klabel::check_sets(set_off, set_labels, n_sets, &where) == klabel::SET_LABEL)
    return fail(c, NEMO_ERR_INVALID, "nemo_witness_labels: the label at position %llu is UINT32_MAX, which is no label",
                (unsigned long long)where);
  std::vector<uint32_t> &desc = cs.wit_desc;  // [n] graphs | the tiers' list positions
  desc.assign(2 * n, 0u);
  for (size_t i = 0; i < n; i++) {
    uint32_t r;
    if ((rc = run_index(c, iters[i], &r))) return rc;
    desc[i] = 2 * r + (uint32_t)cond;
  }
  if (!wit::rows_fit(n, n_sets))
    return fail(c, NEMO_ERR_LIMIT, "nemo_witness_labels: %zu list positions x %zu sets exceed 2^32 - 2 hypotheses in one call: tile the call", n,
                n_sets);
  if (!klabel::words_fit(n, n_sets))
    return fail(c, NEMO_ERR_LIMIT, "nemo_witness_labels: %zu list positions x %llu chunks of 64 sets exceed 2^28 words: tile the call", n,
                (unsigned long long)klabel::chunks(n_sets));
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_whole(c))) return rc;  // may read any graph's build outputs
  if ((rc = ensure_load_checked(c))) return rc;
  cs.wit_n = n, cs.wit_sets = n_sets, cs.wit_chunks = klabel::chunks(n_sets);
  if (!n || !n_sets) {  // zero rows
    cs.wit_done = true;
    return NEMO_OK;
  }
  std::vector<uint64_t> &off = cs.wit_setoff;  // relative to the first set
  off.resize(n_sets + 1);
  for (size_t k = 0; k <= n_sets; k++) off[k] = set_off[k] - set_off[0];
  const uint32_t *lab = n_labels ? set_labels + set_off[0] : nullptr;
  const std::vector<uint32_t> dist = wit::distinct_labels(lab, n_labels);
  cs.wit_ent = wit::rows_of(lab, n_labels, dist);
  cs.wit_ent.insert(cs.wit_ent.end(), dist.begin(), dist.end());
  return wit_run(c, "nemo_witness_labels", n, n_sets, cs.wit_ent.data(), n_labels, (uint32_t)dist.size(), flags);
}

int nemo_fetch_witness(nemo_ctx *c, nemo_witness *out, uint64_t cap, uint64_t *n_out) {
  if (!c) return NEMO_ERR_INVALID;
  if (c->node || !c->cs.wit_done)
    return fail(c, NEMO_ERR_STATE, "nemo_fetch_witness before a witness call (or after a later nemo_load_corpus)");
  const uint64_t n = c->cs.wit_n * c->cs.wit_sets;  // no ensure_whole: reads the last call's host rows, no graph
  if (n_out) *n_out = n;
  if (!out) return NEMO_OK;
  if (cap < n) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  if (n) memcpy(out, c->h_wit.p, n * sizeof(nemo_witness));
  return NEMO_OK;
}

int nemo_fetch_witness_mask(nemo_ctx *c, uint64_t hyp, uint8_t *out, uint64_t cap) {
  if (!c) return NEMO_ERR_INVALID;
  if (c->node || !c->cs.wit_done)
    return fail(c, NEMO_ERR_STATE, "nemo_fetch_witness_mask before a witness call (or after a later nemo_load_corpus)");
  CorpusState &cs = c->cs;
  if (!cs.wit_masks) return fail(c, NEMO_ERR_STATE, "nemo_fetch_witness_mask: the last witness call did not keep its need words (NEMO_WIT_MASKS)");
  const uint64_t n = cs.wit_n * cs.wit_sets;
  if (hyp >= n)
    return fail(c, NEMO_ERR_INVALID, "hypothesis %llu out of range (%llu hypotheses)", (unsigned long long)hyp, (unsigned long long)n);
  const wit::Hyp x = wit::hyp_at(hyp, cs.wit_sets);
  const uint64_t V = cs.nv(cs.wit_desc[x.pos]);
  if (!V) return NEMO_OK;
  if (!out) return NEMO_ERR_INVALID;
  if (cap < V) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<uint64_t> w(V);  // the chunk's words; the hypothesis is one bit column of them
  HIPCHK(c, hipMemcpyAsync(w.data(), cs.d_wtneed.p + wit::need_word0(x, cs.wit_moff.data(), V), V * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (uint64_t v = 0; v < V; v++) out[v] = (uint8_t)((w[v] >> x.bit) & 1u);
  return NEMO_OK;
}

}  // extern "C"
