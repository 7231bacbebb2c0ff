// knock_api.h — the host code the knock-out family's calls share (api_knock.hip, api_cuts.hip, api_klabel.hip,
// api_lcuts.hip, api_gcuts.hip, api_witness.hip): the wait for a call's copies to pinned memory, the fetches' copy of a
// call's host data (the cut, repair and lineage searches' fetches), the dynamic LDS of a persistent
// LDS-tier launch, the listed graphs' split into the two tiers (api_klabel.hip, api_lcuts.hip, api_gcuts.hip), and the
// rounds' sizes and the rows of the cut and repair searches (cut_api.h for api_cuts.hip and api_repair.hip;
// api_lcuts.hip, api_gcuts.hip), and the rounds' limits, launch plans and driver of the two searches by label
// (api_lcuts.hip, api_gcuts.hip).  The searches over one graph share more: cut_api.h.  Every call keeps
// its own event, pinned buffer, device buffers and state (ctx.h); nothing here owns any.  GroupTimer and grow_group
// are ctx.h's.
#pragma once
#include <functional>

#include "ctx.h"

// the copies queued so far have reached pinned memory; ev is the call's own event
static inline int wait_copied(nemo_ctx *c, hipEvent_t ev) {
  HIPCHK(c, hipEventRecord(ev, c->stream));
  HIPCHK(c, hipEventSynchronize(ev));
  return NEMO_OK;
}

// A fetch of the last call's host data (no ensure_whole: no graph is read): n elements of `elem` bytes at src into
// out[cap].  done: the call's result stands; who: the fetch; calls: the calls that make its result.
static inline int fetch_result(nemo_ctx *c, bool done, const char *who, const char *calls, const void *src, uint64_t n, size_t elem, void *out,
                               uint64_t cap, uint64_t *n_out) {
  if (c->node || !done) return fail(c, NEMO_ERR_STATE, "%s before %s (or after a later nemo_load_corpus)", who, calls);
  if (n_out) *n_out = n;
  if (!out) return NEMO_OK;
  if (cap < n) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  if (n) memcpy(out, src, n * elem);
  return NEMO_OK;
}

// ---- a buffer that grows alone inside a call (nemo_lineage_cuts, nemo_lineage_group_cuts) ------------------
// b to `need` elements with its first `keep` elements kept (the frontier behind a grown emission buffer, the cuts
// before a level that could overfill them): a new block, a copy on the stream, a wait, the old block released
template <class T>
static int grow_keep(nemo_ctx *c, DevBuf<T> &b, uint64_t need, uint64_t keep) {
  if (b.p && need <= b.cap) return NEMO_OK;
  DevBuf<T> nb;
  if (int rc = nb.grow(c, need)) return rc;
  if (keep && b.p) HIPCHK(c, hipMemcpyAsync(nb.p, b.p, keep * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  b.release(c);
  b = nb;
  return NEMO_OK;
}

// b to `need` elements, its contents dropped, behind a wait for the stream (an earlier launch may still read it)
template <class T>
static int grow_drop(nemo_ctx *c, DevBuf<T> &b, uint64_t need) {
  if (b.p && need <= b.cap) return NEMO_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return b.grow(c, need);
}

// What a workgroup of k_kl_lds / k_lc_lds takes of a CU's LDS beside its dynamic part: the kernel's static LDS (80
// and 48 bytes by the compiler's report, profiles/r17_kernel_resources.txt), rounded up to whole allocation granules
// with one to spare.  A value too small cannot cost a resident workgroup: ko_lds_total's second query refuses the
// larger size then.
#define KO_LDS_STATIC 512

// The dynamic LDS of a persistent LDS-tier launch: the largest image, and up to `want` bytes more behind it (the
// head of a hit list) as far as a workgroup may take them while as many workgroups stay resident per CU; what does
// not fit goes to the workgroup's region.  resident(bytes): the kernel's resident workgroups on the whole device
// at that much dynamic LDS, 0 for none (it raises the kernel's MaxDynamicSharedMemorySize, a permission, not an
// allocation; the launch sets it to its own size).  *n_res: those workgroups at *total.
template <class R>
static int ko_lds_total(nemo_ctx *c, const char *who, const char *kernel, R &&resident, uint32_t image, uint64_t want, uint32_t lds_static,
                 uint32_t *total, uint32_t *n_res) {
  const uint32_t n_cu = c->cs.dc.n_cu;
  const uint32_t base = resident(image);
  if (!base) return fail(c, NEMO_ERR_HIP, "%s: no workgroup of %s is resident at %u bytes of LDS", who, kernel, image);
  *total = image, *n_res = base;
  int per_cu_lds = 0;
  if (hipDeviceGetAttribute(&per_cu_lds, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, c->device) != hipSuccess) {
    (void)hipGetLastError();
    return NEMO_OK;
  }
  const int64_t room = (int64_t)per_cu_lds / (base / n_cu) - lds_static;
  if (room <= (int64_t)image) return NEMO_OK;
  const uint32_t more = (uint32_t)std::min<uint64_t>((uint64_t)room & ~15ull, image + ((want + 15) & ~15ull));
  if (more > image && resident(more) == base) *total = more;
  return NEMO_OK;
}

// ---- the tiers of a run list (nemo_knockout_labels, nemo_min_label_cuts) --------------------------------
// The graphs' Kahn level counts into cs.kl_nlev, once per load: a function of the loaded graphs.  h / ev: the
// calling entry point's pinned buffer and event.
template <class T>
static int ensure_nlev(nemo_ctx *c, Pinned<T> &h, hipEvent_t ev) {
  CorpusState &cs = c->cs;
  if (!cs.kl_nlev.empty()) return NEMO_OK;
  int rc;
  if ((rc = h.grow(c, 4ull * cs.G / sizeof(T) + 8))) return rc;
  nemo::launch_to_host(h.p, cs.dc.nlev, 4ull * cs.G, c->stream);
  if ((rc = wait_copied(c, ev))) return rc;
  const uint32_t *lv = reinterpret_cast<const uint32_t *>(h.p);
  cs.kl_nlev.assign(lv, lv + cs.G);
  return NEMO_OK;
}

// graph g's tier and its LDS image, by the level counts ensure_nlev read
static inline bool tier_lds(const nemo_ctx *c, uint32_t g) {
  return knock::lds_fits(c->cs.nv(g), c->cs.ne(g), c->cs.kl_nlev[g], c->opt.knock_lds_max);
}
static inline uint32_t tier_image(const nemo_ctx *c, uint32_t g) {
  return knock::knock_lds_bytes((uint32_t)c->cs.nv(g), (uint32_t)c->cs.ne(g), c->cs.kl_nlev[g]);
}

struct Tiers {
  uint32_t n_lds = 0, n_glob = 0;  // list positions of each tier
  uint32_t image = 0;              // the LDS tier's largest image
  uint64_t lds_v = 0, glob_v = 0;  // the most nodes of a graph of each tier
};

// desc[0 .. n) are the listed graphs; desc[n .. 2 n) become the LDS tier's list positions, then the global tier's,
// each in list order.  fits(g) / image(g): the calling family's tier rule and LDS image (the witness calls keep a
// second word array, wit_host.h).
template <class F, class I>
static inline Tiers split_tiers_by(const nemo_ctx *c, std::vector<uint32_t> &desc, size_t n, F &&fits, I &&image) {
  const CorpusState &cs = c->cs;
  Tiers t;
  for (size_t i = 0; i < n; i++) {
    const uint32_t g = desc[i];
    if (fits(g)) t.n_lds++, t.image = std::max<uint32_t>(t.image, image(g)), t.lds_v = std::max(t.lds_v, cs.nv(g));
    else t.n_glob++, t.glob_v = std::max(t.glob_v, cs.nv(g));
  }
  uint32_t l = 0, gl = 0;
  for (size_t i = 0; i < n; i++) {
    if (fits(desc[i])) desc[n + l++] = (uint32_t)i;
    else desc[n + t.n_lds + gl++] = (uint32_t)i;
  }
  return t;
}
// ... by k_ko_lds's image and the option knock_lds_max
static inline Tiers split_tiers(const nemo_ctx *c, std::vector<uint32_t> &desc, size_t n) {
  return split_tiers_by(c, desc, n, [&](uint32_t g) { return tier_lds(c, g); }, [&](uint32_t g) { return tier_image(c, g); });
}

// ---- the rounds of a cut search by label across runs (nemo_min_label_cuts, nemo_min_group_cuts) --------------
// A round's two limits (lcut_host.h) with the calling entry point's name and what it tells the caller to shorten.
static inline int label_round_limit(nemo_ctx *c, const char *who, const char *shorten, size_t n, uint64_t k, uint32_t sz) {
  switch (lcuts::round_check(n, k, sz)) {
    case lcuts::ROUND_HYPS:
      return fail(c, NEMO_ERR_LIMIT, "%s: the sets of %u of %llu live candidates exceed 2^32 - 2 hypotheses: shorten the %s or the run list", who,
                  sz, (unsigned long long)k, shorten);
    case lcuts::ROUND_WORDS:
      return fail(c, NEMO_ERR_LIMIT, "%s: %zu list positions x %llu chunks of 64 sets of %u exceed 2^28 words: shorten the %s or the run list",
                  who, n, (unsigned long long)cuts::chunks(cuts::round_hyps(k, sz)), sz, shorten);
    default:
      return NEMO_OK;
  }
}

struct LabelPlan {  // one round's launches
  uint32_t lds_total = 0;
  uint64_t rw_lds = 0, rw_glob = 0;  // region words of a workgroup
  uint64_t r_lds = 1, r_glob = 1;    // most workgroups
};

// The rounds' LDS and what a workgroup keeps in device memory, for a hit list of `rows` rows (rows + 1 + V entries,
// lcut_host.h) behind the image.  resident(size, bytes): the resident workgroups of round `size`'s LDS-tier kernel;
// lds_static: its static LDS.  *reg_need: the u64 words of all regions of the largest launch.
template <class R>
static int label_plans(nemo_ctx *c, const char *who, const char *kernel, R &&resident, const std::vector<uint32_t> &desc, size_t n,
                       const Tiers &tr, uint64_t rows, uint32_t lds_static, uint32_t max_size, LabelPlan *plan, uint64_t *reg_need) {
  const CorpusState &cs = c->cs;
  const uint32_t cap = c->opt.kl_grid;
  *reg_need = 1;
  for (uint32_t sz = 1; sz <= max_size; sz++) {
    LabelPlan &p = plan[sz - 1];
    uint32_t res_lds = 1;
    if (tr.n_lds) {
      if (int rc = ko_lds_total(c, who, kernel, [&](uint32_t b) { return resident(sz, b); }, tr.image, 4 * lcuts::list_entries(rows, tr.lds_v),
                                lds_static, &p.lds_total, &res_lds))
        return rc;
      for (size_t k = 0; k < tr.n_lds; k++) {
        const uint32_t g = desc[desc[n + k]];
        p.rw_lds = std::max(p.rw_lds, lcuts::region_words(0, lcuts::list_entries(rows, cs.nv(g)), (p.lds_total - tier_image(c, g)) / 4u));
      }
    }
    p.rw_glob = lcuts::region_words(knock::dead_words(tr.glob_v), lcuts::list_entries(rows, tr.glob_v), 0);
    p.r_lds = klabel::region_grid(res_lds, p.rw_lds), p.r_glob = klabel::region_grid(2ull * cs.dc.n_cu, p.rw_glob);
    if (cap) p.r_lds = std::min<uint64_t>(p.r_lds, cap), p.r_glob = std::min<uint64_t>(p.r_glob, cap);
    if (tr.n_lds) *reg_need = std::max(*reg_need, p.r_lds * p.rw_lds);
    if (tr.n_glob) *reg_need = std::max(*reg_need, p.r_glob * p.rw_glob);
  }
  return NEMO_OK;
}

// One round: the two tiers' sweeps, then k_lc_reduce.  r: the round (size, n, n_hyp, n_chunks and the buffers set);
// d_desc: the device copy of desc.  launch_lds(grid) / launch_glob(grid) launch the call's own sweep on r, timed
// under lds_name / glob_name.  The byte model: a work item reads its graph's image (4 E + 12 V + 4 L + 8) and its
// 4 V labels twice (count, scatter); a chunk writes 8 bytes (round 1: 16) and reads chunk_bytes more (the call's own:
// what its 64 sets name); ops = E child words per chunk, an upper bound (the host does not know which chunks hit
// nothing and skip the sweep); the global tier adds 16 V per chunk for its dead words in device memory.  The
// reduction reads every word once and writes one per chunk.
template <class LL, class LG>
static int label_round(nemo_ctx *c, const LabelPlan &p, const Tiers &tr, const std::vector<uint32_t> &desc, nemo::LcArgs &r,
                       const uint32_t *d_desc, double chunk_bytes, const char *lds_name, const char *glob_name, LL &&launch_lds,
                       LG &&launch_glob, double *bytes, double *ops) {
  if (!r.n_chunks) return NEMO_OK;
  const CorpusState &cs = c->cs;
  const uint32_t cap = c->opt.kl_grid, n = r.n;
  const uint64_t ck = r.n_chunks;
  const double per_word = r.size == 1 ? 16.0 : 8.0;
  for (int tier = 0; tier < 2; tier++) {
    const uint32_t nt = tier ? tr.n_glob : tr.n_lds;
    if (!nt) continue;
    const uint64_t res = tier ? p.r_glob : p.r_lds;
    const klabel::Split sp = klabel::split(nt, ck, res);
    const uint32_t grid = klabel::grid(sp.items, res, cap);
    double b = 0, o = 0;
    for (uint32_t k = 0; k < nt; k++) {
      const uint32_t g = desc[desc[n + (tier ? tr.n_lds : 0) + k]];
      const double V = (double)cs.nv(g), E = (double)cs.ne(g), L = (double)cs.kl_nlev[g];
      b += sp.parts * (4.0 * E + 12.0 * V + 4.0 * L + 8.0 + 8.0 * V) + (double)ck * (per_word + chunk_bytes + (tier ? 16.0 * V : 0.0));
      o += (double)ck * E;
    }
    r.pos = d_desc + n + (tier ? tr.n_lds : 0);
    r.n_tier = nt, r.parts = sp.parts;
    r.lds_total = tier ? 0u : p.lds_total;
    r.region_words = tier ? p.rw_glob : p.rw_lds;
    r.dead_words = tier ? knock::dead_words(tr.glob_v) : 0;
    int rc;
    if (tier) rc = timed(c, glob_name, b, o, [&] { launch_glob(grid); });
    else rc = timed(c, lds_name, b, o, [&] { launch_lds(grid); });
    if (rc) return rc;
    *bytes += b, *ops += o;
  }
  const double b_red = per_word * (double)n * (double)ck + per_word * (double)ck;
  *bytes += b_red;
  return timed(c, "k_lc_reduce", b_red, 0, [&] { nemo::launch_lc_reduce(r, c->stream); });
}

// ---- the rounds and the rows of a cut search (nemo_min_cuts, nemo_min_label_cuts) -----------------------
struct CutRounds {  // rounds 1 to 3 once round 1 has left K1 live candidates of K
  uint64_t K = 0, K1 = 0;
  uint64_t n_hyp[3] = {0, 0, 0}, ck[3] = {0, 0, 0};  // hypotheses and chunks of 64
  uint64_t scan_off[3] = {0, 0, 0}, n_scan = 0;      // the rounds' [chunks + 1] scans in the scan buffer
  uint64_t scan_need = 0;                            // ... and its size with launch_scan's tile sums behind them
};

// limit(K1, size): the call's own check of a later round, with its own message; 0 if the round fits.  Per round,
// before the round's launch: K1 is known only now.
template <class L>
static int cut_rounds(uint64_t K, uint64_t K1, uint32_t max_size, L &&limit, CutRounds *r) {
  r->K = K, r->K1 = K1, r->n_hyp[0] = K;
  for (uint32_t sz = 2; sz <= max_size; sz++) {
    if (int rc = limit(K1, sz)) return rc;
    r->n_hyp[sz - 1] = cuts::round_hyps(K1, sz);
  }
  for (int k = 0; k < 3; k++) r->ck[k] = cuts::chunks(r->n_hyp[k]);
  r->scan_off[1] = r->ck[0] + 1, r->scan_off[2] = r->ck[0] + r->ck[1] + 2;
  r->n_scan = r->ck[0] + r->ck[1] + r->ck[2] + 3;
  r->scan_need = r->n_scan + nemo::dx_scan_tiles((uint32_t)(std::max(r->ck[0], std::max(r->ck[1], r->ck[2])) + 1));
  return NEMO_OK;
}

struct CutOut {               // where a cut search's rows go: the call's own buffers, event and state
  Pinned<uint32_t> &h;        // pinned: the totals, then the rows
  hipEvent_t ev;
  DevBuf<uint32_t> &d_scan;   // CutRounds::scan_need entries
  DevBuf<uint32_t> &d_rows;   // grows alone, once the totals are known
  uint32_t width;             // u32 words a row takes in d_rows and h: 4 for [rows][4]; 5 with a [rows] column behind them
  uint64_t *stats, *rows;     // the call's nine stats and row count
  bool *done;
};

// The rows of a cut search whose rounds' words are in place (e[k]: size, n_hyp, n_chunks, words, cand, live):
// k_cuts.hip's row kernels count and scan the words' popcounts, the totals come back in one blocking round trip, the
// rows are written in (size, rank) order and copied to pinned memory, the stats and the row count go to the call's
// state.  after_emit(k, found, base, rows, &bytes), if set, follows round k's emit: its `found` rows start at row
// `base` of `rows` (nemo_min_label_cuts recounts their support).  Ends the call's timing group.
static inline int cut_rows(nemo_ctx *c, const CutOut &o, const CutRounds &r, nemo::CutArgs *e, uint32_t max_size, GroupTimer &timer,
                    double bytes, double ops,
                    const std::function<int(uint32_t, uint64_t, uint64_t, uint64_t, double *)> &after_emit = nullptr) {
  hipStream_t s = c->stream;
  int rc;
  uint32_t *tsum = o.d_scan.p + r.n_scan;
  nemo::HostCopies hc;
  for (uint32_t k = 0; k < max_size; k++) {
    if (!e[k].n_chunks) continue;
    e[k].scan = o.d_scan.p + r.scan_off[k];
    const double b = 12.0 * e[k].n_chunks;
    if ((rc = timed(c, "k_cut_count", b, 0, [&] { nemo::launch_cut_count(e[k], s); }))) return rc;
    if ((rc = timed(c, "k_cut_scan", 16.0 * e[k].n_chunks, 0, [&] { nemo::launch_scan(e[k].scan, e[k].n_chunks + 1, tsum, s); })))
      return rc;
    bytes += b + 16.0 * e[k].n_chunks;
    hc.add(o.h.p + k, e[k].scan + e[k].n_chunks, 4);
  }
  o.h.p[0] = o.h.p[1] = o.h.p[2] = 0;
  nemo::launch_to_host_multi(hc, s);
  if ((rc = wait_copied(c, o.ev))) return rc;
  const uint64_t found[3] = {o.h.p[0], o.h.p[1], o.h.p[2]};
  const uint64_t rows = found[0] + found[1] + found[2];
  if (rows) {
    if (o.width * rows > o.d_rows.cap || !o.d_rows.p) {
      HIPCHK(c, hipStreamSynchronize(s));
      if ((rc = o.d_rows.grow(c, o.width * rows))) return rc;
    }
    if ((rc = o.h.grow(c, o.width * rows))) return rc;
    uint64_t base = 0;
    for (uint32_t k = 0; k < max_size; k++) {
      if (!e[k].n_chunks || !found[k]) continue;
      e[k].rows = o.d_rows.p + 4 * base;
      const double b = 12.0 * e[k].n_chunks + 16.0 * (double)found[k] + 8.0 * (k + 1) * (double)found[k];
      if ((rc = timed(c, "k_cut_emit", b, 0, [&] { nemo::launch_cut_emit(e[k], s); }))) return rc;
      bytes += b;
      if (after_emit && (rc = after_emit(k, found[k], base, rows, &bytes))) return rc;
      base += found[k];
    }
  }
  timer.done(bytes, ops);
  if (rows) {
    nemo::launch_to_host(o.h.p, o.d_rows.p, 4ull * o.width * rows, s);
    if ((rc = wait_copied(c, o.ev))) return rc;
  }
  for (uint32_t k = 0; k < max_size; k++) {
    o.stats[3 * k] = k ? r.K1 : r.K;
    o.stats[3 * k + 1] = r.n_hyp[k];
    o.stats[3 * k + 2] = found[k];
  }
  *o.rows = rows;
  *o.done = true;
  return NEMO_OK;
}
