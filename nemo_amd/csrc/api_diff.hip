// api_diff.hip — differential provenance: nemo_diffprov*, the symmetric diff, the pair diff and their fetches.
#include "ctx.h"

extern "C" {

// d_labels != NULL: label mode, every entry's failGoals is the device label
// set [n, label...] (n <= labels_cap), e.g. broadcast from the shard that owns
// failedRuns[0]; mode is then ignored.
static int diffprov_impl(nemo_ctx *c, const uint32_t *failed_iters, size_t n_failed, int mode,
                         const uint32_t *d_labels, uint64_t labels_cap) {
  if (!c || (!failed_iters && n_failed)) return NEMO_ERR_INVALID;
  if (mode != NEMO_DIFF_REFERENCE && mode != NEMO_DIFF_PER_RUN) return fail(c, NEMO_ERR_INVALID, "unknown diff mode %d", mode);
  if (!c->cs.loaded) return fail(c, NEMO_ERR_STATE, "nemo_diffprov without a loaded corpus (the last load failed?)");
  if (!c->cs.marked) return fail(c, NEMO_ERR_STATE, "nemo_diffprov before nemo_mark_holds");
  // (the diff kernels read no holds flags: a deferred mark stays fused with the simplification)
  HIPCHK(c, hipSetDevice(c->device));
  if (int rw = ensure_run0(c)) return rw;  // reads the build outputs of run 0's graphs only
  c->cs.n_entries = 0;
  c->cs.dc_done = false;  // the classes were those of the previous call's masks
  c->cs.diff_done = n_failed == 0 || c->cs.run0 < 0;
  if (c->cs.diff_done) return NEMO_OK;  // MATCH on run 0 finds nothing
  if (int re = ensure_event(c, &c->ev_up_dsrc)) return re;
  HIPCHK(c, hipEventSynchronize(c->ev_up_dsrc));  // the previous upload has landed (at once if there was none)
  if (int rg = c->h_dsrc.grow(c, 3 * n_failed)) return rg;
  // D_f depends on run 0 and on the label source alone (differential-provenance.go:22-43):
  // entries with the same source share one computation.  In the reference mode every
  // entry's source is failedRuns[0] (the in-place ###RUN### substitution of :43), so
  // the whole call is one computation; in the per-run mode each distinct failed run is.
  uint32_t *src = c->h_dsrc.p, *emap = c->h_dsrc.p + n_failed, *urep = c->h_dsrc.p + 2 * n_failed;
  c->cs.dmap.assign(n_failed, 0);
  std::unordered_map<uint32_t, uint32_t> uniq;
  uint32_t nu = 0;
  double src_bytes = 0;  // the label sources' HBM reads (word + label per node, or the label set)
  for (size_t e = 0; e < n_failed; e++) {
    uint32_t r;
    const uint32_t it = mode == NEMO_DIFF_PER_RUN && !d_labels ? failed_iters[e] : failed_iters[0];
    int rc = run_index(c, d_labels ? failed_iters[e] : it, &r);
    if (rc) return rc;
    const uint32_t key = d_labels ? 0u : 2 * r + 1;  // label mode: one set for every entry
    auto ins = uniq.emplace(key, nu);
    if (ins.second) {
      urep[nu] = (uint32_t)e;  // the first entry of each source stands for it (nemo_pull_edges(2))
      src[nu++] = 2 * r + 1;
      src_bytes += d_labels ? 0.0 : 8.0 * (double)c->cs.nv(2 * r + 1);
    }
    c->cs.dmap[e] = emap[e] = ins.first->second;
  }
  if (d_labels) src_bytes = 4.0 * (double)labels_cap;  // read once, then L2-resident
  const bool expand = nu < n_failed;
  CorpusState &cs = c->cs;
  const uint64_t V0 = cs.V0(), E0 = cs.E0();
  const bool dx = c->cs.dx_ok && !c->opt.diff_legacy && (c->opt.diff_window != 2 || c->cs.g0_maxdeg <= nemo::dx_max_row_tiny());
  int rc;
  // capacities in whole 64-entry chunks: the per-entry buffers of corpora (batches) with a few more
  // or fewer failed runs are the same size, so the allocation cache hands the same blocks back (a
  // block no load takes is freed at the next load, and hipFree waits for the whole device)
  const uint64_t nf_cap = (n_failed + 63) & ~(uint64_t)63;
  auto drop_legacy = [&] { cs.d_dbits.release(c), cs.d_dumask.release(c), cs.d_ddepth.release(c), cs.d_dtopo.release(c); };
  if (3 * nf_cap > cs.d_dsrc.cap || !cs.d_miss.p) {
    cs.d_dsrc.release(c), cs.d_dmask.release(c), cs.d_miss.release(c);
    drop_legacy();  // a larger entry count outgrows it too: it comes back at the next call that needs it
    if ((rc = cs.d_dsrc.grow(c, 3 * nf_cap)) || (rc = cs.d_dmask.grow(c, nf_cap * V0)) ||
        (rc = cs.d_miss.grow(c, 2 * nf_cap * (V0 + 1))))
      return rc;
  }
  if (!dx && (nf_cap * V0 > cs.d_dbits.cap || !cs.d_dtopo.p)) {  // the one-workgroup-per-entry kernels' scratch
    drop_legacy();
    if ((rc = cs.d_dbits.grow(c, nf_cap * V0)) || (rc = cs.d_dumask.grow(c, nf_cap * V0)) ||
        (rc = cs.d_ddepth.grow(c, nf_cap * V0)) || (rc = cs.d_dtopo.grow(c, 4 * V0 + 2 * E0 + 2 + cs.n_r0lab)))
      return rc;
  }
  const uint32_t nch = (nu + 63) / 64, w32 = (uint32_t)((V0 + 31) / 32), nu_cap = 64 * nch;
  if (dx && nu > cs.dx_nu_cap) {
    cs.d_dxpb.release(c), cs.d_dxsval.release(c), cs.d_dxlpl.release(c), cs.d_dxw.release(c), cs.d_dxfb.release(c);
    cs.dx_nu_cap = 0;
    if ((rc = cs.d_dxpb.grow(c, (uint64_t)nu_cap * w32)) || (rc = cs.d_dxsval.grow(c, (uint64_t)nu_cap * V0)) ||
        (rc = cs.d_dxlpl.grow(c, (uint64_t)nu_cap + nch)) ||  // maxima, then the chunks' walk flags
        (rc = cs.d_dxw.grow(c, 4 * (uint64_t)nch * V0)) ||
        (rc = cs.d_dxfb.grow(c, 8 * (uint64_t)nch * V0)))  // 32 bytes per position and chunk
      return rc;
    cs.dx_nu_cap = nu_cap;
  }
  if ((rc = cs.d_nmiss.grow(c, 1))) return rc;
  c->cs.d_dmap = c->cs.d_dsrc.p + n_failed;
  c->cs.n_uniq = nu;
  // the diff kernels go on `aux` once `stream` has reached this point (the load /
  // rebuild of the graphs they read is queued there)
  hipStream_t s = c->stream;
  if (c->opt.diff_on_aux) {
    if (!c->aux) HIPCHK(c, hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking));
    if ((rc = ensure_event(c, &c->ev_fork))) return rc;
    HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->aux, c->ev_fork, 0));
    s = c->aux;
  }
  nemo::launch_to_host(c->cs.d_dsrc.p, src, 3 * n_failed * 4, s);  // pinned -> device by a copy kernel (no blit queue)
  HIPCHK(c, hipEventRecord(c->ev_up_dsrc, s));
  nemo::launch_zero(c->cs.d_nmiss.p, 4, s);
  // HBM lower bound: run 0's post graph once (rows both ways, node word, Kahn
  // order: 8E0 + 16V0 -- every entry re-reads it from L2), each distinct label
  // source and each entry's D mask (V0); the three reachability sweeps per
  // computed entry are counted as traversed edges, not as HBM bytes
  const double bytes = 8.0 * E0 + 16.0 * V0 + src_bytes + (double)n_failed * V0;
  c->cs.dx_last = dx;
  if (dx) {
    nemo::DxArgs a{};
    a.p = c->cs.dxp;
    a.nu = nu;
    a.nch = nch;
    a.src = c->cs.d_dsrc.p;
    a.ref_labels = d_labels;
    a.r0lab = c->cs.d_r0lab;
    a.r0hkey = c->cs.d_r0hkey;
    a.r0hval = c->cs.d_r0hval;
    a.r0hmask = c->cs.r0hmask;
    a.r0dense = c->cs.dxp.r0dense;
    a.nlab = c->cs.nlab;
    a.pb = c->cs.d_dxpb.p;
    a.w32 = w32;
    uint64_t maxsrc = d_labels ? labels_cap : 0;
    for (uint32_t u = 0; u < nu && !d_labels; u++)
      maxsrc = std::max<uint64_t>(maxsrc, cs.nv(src[u]));
    a.lab_per = 8192;  // one workgroup per source up to 8192 nodes: its bitmap stored whole, no atomics
    a.lab_split = (uint32_t)std::max<uint64_t>(1, (maxsrc + a.lab_per - 1) / a.lab_per);
    const size_t plane = (size_t)nch * V0;
    a.gw = c->cs.d_dxw.p;
    a.bw = a.gw + plane;
    a.dw = a.bw + plane;
    a.lw = a.dw + plane;
    a.fb = reinterpret_cast<uint8_t *>(c->cs.d_dxfb.p);
    a.sval = c->cs.d_dxsval.p;
    a.maxlen = c->cs.d_dxlpl.p;
    a.wflag = c->cs.d_dxlpl.p + c->cs.dx_nu_cap;
    a.mask = c->cs.d_dmask.p;
    a.map = c->cs.d_dmap;
    a.n_entries = (uint32_t)n_failed;
    a.missing = c->cs.d_miss.p;
    a.n_missing = c->cs.d_nmiss.p;
    a.window = c->opt.diff_window;
    a.legacy_lp = c->opt.diff_unfused;
    a.urep = c->cs.d_dsrc.p + 2 * n_failed;
    a.own_mask = nu == n_failed ? 1u : 0u;
    if (c->cs.dx_img_key < 0) {
      // g0 in Kahn order (read the Kahn order, both CSRs and the node words;
      // write positions, rows both ways, level bounds), once per load / rebuild
      c->cs.dxp.err0 = c->cs.dc.err + c->cs.dxp.g0;
      if ((rc = timed_on(c, s, "k_dxprep", 16.0 * E0 + 44.0 * V0, 0,
                         [&] { nemo::launch_dx_prep(c->cs.dc, c->cs.dxp, c->cs.dx_its.tsum, s); })))
        return rc;
    }
    if (c->cs.dx_img_key != (int)c->opt.diff_window) {
      // the walk images (read rows and Kahn levels, write records, steps and
      // misses), once per load / rebuild and window configuration (test knob)
      nemo::dx_img_configs(c->cs.dxp.V0, c->cs.dxp.E0, c->opt.diff_window, c->cs.dx_img);
      if ((rc = timed_on(c, s, "k_dximg", 2 * (16.0 * E0 + 32.0 * V0), 0,
                         [&] { nemo::launch_dx_img(c->cs.dxp, c->cs.dx_img, c->cs.dx_its, s); })))
        return rc;
      c->cs.dx_img_key = (int)c->opt.diff_window;
    }
    for (int k = 0; k < 2; k++) a.img[k] = c->cs.dx_img[k];
    rc = timed_on(c, s, "k_diff", bytes, (double)nu * 3 * E0, [&] { nemo::launch_dx(c->cs.dc, a, s); });
  } else {
    nemo::DiffArgs a;
    a.g0 = cs.g0();
    a.src = c->cs.d_dsrc.p;
    a.ref_labels = d_labels;
    a.r0lab = c->cs.d_r0lab;
    a.r0idx = c->cs.d_r0idx;
    a.n_r0lab = c->cs.n_r0lab;
    a.r0hkey = c->cs.d_r0hkey;
    a.r0hval = c->cs.d_r0hval;
    a.r0hmask = c->cs.r0hmask;
    a.bits = c->cs.d_dbits.p;
    a.depth = c->cs.d_ddepth.p;
    a.tpos = c->cs.d_dtopo.p;
    a.tinfo = a.tpos + V0;
    a.trp = a.tinfo + V0;
    a.tfp = a.trp + V0 + 1;
    a.trc = a.tfp + V0 + 1;
    a.tfc = a.trc + E0;
    a.r0pos = a.tfc + E0;
    a.mask = expand ? c->cs.d_dumask.p : c->cs.d_dmask.p;
    a.missing = c->cs.d_miss.p;
    a.n_missing = c->cs.d_nmiss.p;
    rc = timed_on(c, s, "k_diff", bytes, (double)nu * 3 * E0,
                  [&] {
                    // the Kahn-order relayout only when g0 may fall outside the LDS tier
                    const bool lds = c->cs.dc.t_diff.bytes && V0 <= c->cs.dc.t_diff.v && E0 <= c->cs.dc.t_diff.e;
                    nemo::launch_diff(c->cs.dc, a, nu, lds ? 0u : (uint32_t)V0, s);
                    if (expand) nemo::launch_diff_expand(c->cs.d_dmask.p, c->cs.d_dumask.p, c->cs.d_dmap, V0, (uint32_t)n_failed, s);
                  });
  }
  if (rc) return rc;
  // D masks and the missing-event count -> pinned host
  if ((rc = ensure_event(c, &c->ev_diff))) return rc;
  if ((rc = c->h_mask.grow(c, n_failed * V0))) return rc;
  if ((rc = c->h_nmiss.grow(c, (uint64_t)1))) return rc;
  // the missing rows too, at the last call's count: nemo_fetch_missing then needs no round
  // trip of its own unless this call found more (d_miss holds n_failed (V0 + 1) rows)
  c->cs.mrows_staged = std::min<uint64_t>(c->mrows_hint, (uint64_t)n_failed * (V0 + 1));
  if ((rc = c->h_mrows.grow(c, 2 * c->cs.mrows_staged + 2))) return rc;
  nemo::HostCopies hc;
  hc.add(c->h_mask.p, c->cs.d_dmask.p, n_failed * V0);
  hc.add(c->h_nmiss.p, c->cs.d_nmiss.p, 4);
  hc.add(c->h_mrows.p, c->cs.d_miss.p, 8 * c->cs.mrows_staged);
  nemo::launch_to_host_multi(hc, s);
  HIPCHK(c, hipEventRecord(c->ev_diff, s));
  c->cs.aux_pending = true;
  c->cs.diff_stream = s;
  c->cs.n_entries = (uint32_t)n_failed;
  c->cs.diff_done = true;
  return NEMO_OK;
}

int nemo_diffprov(nemo_ctx *c, const uint32_t *failed_iters, size_t n_failed, int mode) {
  DISPATCH(node_diffprov(c, failed_iters, n_failed, mode));
  return diffprov_impl(c, failed_iters, n_failed, mode, nullptr, 0);
}

int nemo_diffprov_labels(nemo_ctx *c, const uint32_t *failed_iters, size_t n_failed, const uint32_t *d_labels,
                         uint64_t labels_cap) {
  DISPATCH(node_diffprov_labels(c, failed_iters, n_failed, d_labels, labels_cap));
  if (!d_labels) return c ? fail(c, NEMO_ERR_INVALID, "no label set") : NEMO_ERR_INVALID;
  return diffprov_impl(c, failed_iters, n_failed, NEMO_DIFF_REFERENCE, d_labels, labels_cap);
}

int nemo_diffprov_host_labels(nemo_ctx *c, const uint32_t *failed_iters, size_t n_failed, const uint32_t *labels,
                              uint64_t n_labels) {
  DISPATCH(node_diffprov_host_labels(c, failed_iters, n_failed, labels, n_labels));
  if (!c || (!labels && n_labels)) return NEMO_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = join_aux(c))) return rc;  // the previous diff may still read d_hlab
  if (n_labels + 1 > c->cs.d_hlab.cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((rc = c->cs.d_hlab.grow(c, n_labels + 1))) return rc;
  }
  if ((rc = ensure_event(c, &c->ev_up_hlab))) return rc;
  HIPCHK(c, hipEventSynchronize(c->ev_up_hlab));  // the previous upload has landed (at once if there was none)
  if ((rc = c->h_hlab.grow(c, n_labels + 1))) return rc;
  c->h_hlab.p[0] = (uint32_t)n_labels;
  if (n_labels) memcpy(c->h_hlab.p + 1, labels, n_labels * 4);
  nemo::launch_to_host(c->cs.d_hlab.p, c->h_hlab.p, (n_labels + 1) * 4, c->stream);  // pinned -> device by a copy kernel
  HIPCHK(c, hipEventRecord(c->ev_up_hlab, c->stream));
  return diffprov_impl(c, failed_iters, n_failed, NEMO_DIFF_REFERENCE, c->cs.d_hlab.p, n_labels + 1);
}

int nemo_goal_labels(nemo_ctx *c, uint32_t iteration, int cond, uint32_t *d_out, uint64_t cap) {
  DISPATCH(node_goal_labels(c, iteration, cond, d_out, cap));
  if (!c || !d_out || (cond != 0 && cond != 1)) return NEMO_ERR_INVALID;
  if (!c->cs.loaded) return fail(c, NEMO_ERR_STATE, "no corpus loaded");
  HIPCHK(c, hipSetDevice(c->device));
  if (int rw = ensure_run0(c)) return rw;  // reads the build outputs of run 0's graphs only
  if (int rl = ensure_load_checked(c)) return rl;
  uint32_t r;
  int rc = run_index(c, iteration, &r);
  if (rc) return rc;
  const uint32_t g = 2 * r + (uint32_t)cond;
  const uint64_t V = c->cs.nv(g);
  if (cap < V + 1) return fail(c, NEMO_ERR_INVALID, "label capacity %llu < %llu", (unsigned long long)cap,
                               (unsigned long long)(V + 1));
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = join_aux(c))) return rc;  // d_out may be the label set a previous diff still reads
  return timed(c, "k_goal_labels", 8.0 * (double)V, 0, [&] { nemo::launch_goal_labels(c->cs.dc, g, d_out, c->stream); });
}

int nemo_fetch_diff_mask(nemo_ctx *c, uint32_t entry, uint8_t *out, uint64_t cap) {
  DISPATCH(node_fetch_diff_mask(c, entry, out, cap));
  if (!c || !out) return NEMO_ERR_INVALID;
  if (entry >= c->cs.n_entries) return fail(c, NEMO_ERR_INVALID, "diff entry %u out of range", entry);
  const uint64_t V0 = c->cs.V0();
  if (cap < V0) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  HIPCHK(c, hipSetDevice(c->device));
  if (int rw = ensure_run0(c)) return rw;  // reads the build outputs of run 0's graphs only
  HIPCHK(c, hipEventSynchronize(c->ev_diff));
  memcpy(out, c->h_mask.p + (size_t)entry * V0, V0);
  return NEMO_OK;
}

int nemo_fetch_diff_masks(nemo_ctx *c, uint8_t *out, uint64_t cap) {
  DISPATCH(node_fetch_diff_masks(c, out, cap));
  if (!c || !out) return NEMO_ERR_INVALID;
  if (!c->cs.n_entries) return NEMO_OK;
  const uint64_t n = (uint64_t)c->cs.n_entries * c->cs.V0();
  if (cap < n) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  HIPCHK(c, hipSetDevice(c->device));
  if (int rw = ensure_run0(c)) return rw;  // reads the build outputs of run 0's graphs only
  HIPCHK(c, hipEventSynchronize(c->ev_diff));
  memcpy(out, c->h_mask.p, n);
  return NEMO_OK;
}

int nemo_diff_masks_view(nemo_ctx *c, const uint8_t **masks, uint64_t *n_entries, uint64_t *v0) {
  DISPATCH(node_diff_masks_view(c, masks, n_entries, v0));
  if (!c || !masks) return NEMO_ERR_INVALID;
  *masks = nullptr;
  if (n_entries) *n_entries = c->cs.n_entries;
  if (v0) *v0 = c->cs.V0();
  if (!c->cs.n_entries) return NEMO_OK;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rw = ensure_run0(c)) return rw;  // reads the build outputs of run 0's graphs only
  HIPCHK(c, hipEventSynchronize(c->ev_diff));
  *masks = c->h_mask.p;
  return NEMO_OK;
}

int nemo_fetch_missing(nemo_ctx *c, nemo_missing *out, uint64_t cap, uint64_t *n_out) {
  DISPATCH(node_fetch_missing(c, out, cap, n_out));
  if (!c) return NEMO_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rw = ensure_run0(c)) return rw;  // reads the build outputs of run 0's graphs only
  uint32_t nu_rows = 0;
  if (c->cs.n_entries) {
    HIPCHK(c, hipEventSynchronize(c->ev_diff));
    nu_rows = *c->h_nmiss.p;
    // the fused walks' bounded hand-off wait (k_dx.hip dx_publish) gave up: the rows are void
    if (c->cs.dx_last && (nu_rows & DX_ERR_HANDOFF))
      return fail(c, NEMO_ERR_INVALID, "diff walks: a longest-path workgroup timed out waiting for its Bwd* hand-off");
    nu_rows &= DX_ROWS;
  }
  // rows of the distinct computations (unique index, rule), then one copy per entry
  int rc;
  if ((rc = ensure_event(c, &c->ev_misc))) return rc;
  if (nu_rows > c->cs.mrows_staged) {  // more rows than diffprov copied with the masks
    if ((rc = c->h_mrows.grow(c, 2 * (uint64_t)nu_rows + 2))) return rc;
    if ((rc = join_aux(c))) return rc;
    nemo::launch_to_host(c->h_mrows.p, c->cs.d_miss.p, 8ull * nu_rows, c->stream);
    HIPCHK(c, hipEventRecord(c->ev_misc, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev_misc));
    c->cs.mrows_staged = nu_rows;
  }
  c->mrows_hint = std::max<uint64_t>(256, nu_rows);
  const uint32_t *rows = c->h_mrows.p;
  std::vector<std::vector<uint32_t>> per(c->cs.n_uniq);
  for (uint32_t i = 0; i < nu_rows; i++) per[rows[2 * i]].push_back(rows[2 * i + 1]);
  uint64_t n = 0;
  for (auto &v : per) std::sort(v.begin(), v.end());
  for (uint32_t e = 0; e < c->cs.n_entries; e++) n += per[c->cs.dmap[e]].size();
  if (n_out) *n_out = n;
  if (!out) return NEMO_OK;
  if (cap < n) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  uint64_t k = 0;
  for (uint32_t e = 0; e < c->cs.n_entries; e++)
    for (uint32_t r : per[c->cs.dmap[e]]) {
      out[k].entry = e;
      out[k].rule = r;
      k++;
    }
  return NEMO_OK;
}

// ---- failure classes (DESIGN.md §Failure classes) ----
// The D masks stay in HBM: k_dclass_hash reads the row of every distinct label source once (the
// other entries share it through dmap), the host buckets the 128-bit hashes (dclass_host.h) and
// k_dclass_cmp confirms every bucket member against its bucket's candidate, round by round.  The
// kernels are queued behind the diff kernels on the stream those ran on (`aux` or the context's);
// nothing here waits for ev_diff or reads h_mask.
int nemo_diff_classes(nemo_ctx *c) {
  DISPATCH(node_diff_classes(c));
  if (!c) return NEMO_ERR_INVALID;
  CorpusState &cs = c->cs;
  if (!cs.loaded) return fail(c, NEMO_ERR_STATE, "nemo_diff_classes without a loaded corpus");
  if (!cs.diff_done) return fail(c, NEMO_ERR_STATE, "nemo_diff_classes before nemo_diffprov");
  cs.dc_done = false;
  cs.dc_class_of.clear();
  cs.dc_classes.clear();
  cs.dc_hash.clear();
  cs.dc_rounds = 0;
  const uint32_t n = cs.n_entries, nu = cs.n_uniq;
  const uint64_t V0 = cs.V0();
  cs.dc_support.assign(V0, 0);
  if (!n) {
    cs.dc_done = true;
    return NEMO_OK;
  }
  HIPCHK(c, hipSetDevice(c->device));
  if (int rw = ensure_whole(c)) return rw;  // may read any graph
  int rc;
  if ((rc = ensure_event(c, &c->ev_dclass))) return rc;
  hipStream_t s = cs.diff_stream;  // behind the diff kernels, on whichever stream they ran
  const uint32_t cap = (nu + 63u) & ~63u;
  if (cap > cs.dc_cap) {
    cs.d_dcacc.release(c), cs.d_dcin.release(c), cs.d_dcv.release(c);
    cs.dc_cap = 0;
    if ((rc = cs.d_dcacc.grow(c, 5 * (uint64_t)cap + V0)) || (rc = cs.d_dcin.grow(c, 2 * (uint64_t)cap)) ||
        (rc = cs.d_dcv.grow(c, cap)))
      return rc;
    cs.dc_cap = cap;
  }
  if ((rc = c->h_dcin.grow(c, 2 * (uint64_t)cap))) return rc;
  if ((rc = c->h_dcout.grow(c, 5 * (uint64_t)cap + V0))) return rc;
  // every call ends with its last copy landed (below), so the staging buffers are free here
  std::vector<uint32_t> first(nu, 0);  // source -> its first entry (urep; dmap numbers sources in that order)
  for (uint32_t u = 0; u < nu; u++) c->h_dcin.p[u] = 0;
  for (uint32_t e = n; e-- > 0;) {
    c->h_dcin.p[cs.dmap[e]]++;
    first[cs.dmap[e]] = e;
  }
  nemo::DclassArgs a{};
  a.mask = cs.d_dmask.p;
  a.V0 = V0;
  a.row = cs.d_dsrc.p + 2 * (size_t)n;
  a.weight = cs.d_dcin.p;
  a.nu = nu;
  a.rows_per_block = nemo::dclass_rows_per_block(V0, nu);
  a.hash = reinterpret_cast<uint64_t *>(cs.d_dcacc.p);
  a.pop = cs.d_dcacc.p + 4 * (size_t)cs.dc_cap;
  a.support = cs.d_dcacc.p + 5 * (size_t)cs.dc_cap;
  nemo::launch_to_host(cs.d_dcin.p, c->h_dcin.p, 4ull * nu, s);  // pinned -> device by a copy kernel
  nemo::launch_zero(cs.d_dcacc.p, 4 * (5 * (uint64_t)cs.dc_cap + V0), s);
  // algorithmic bytes: every distinct row once, 20 bytes per source and the support written
  if ((rc = timed_on(c, s, "k_dclass", (double)nu * V0 + 24.0 * nu + 4.0 * V0, 0,
                     [&] { nemo::launch_dclass_hash(a, s); })))
    return rc;
  uint32_t *h_hash = c->h_dcout.p, *h_pop = h_hash + 4 * (size_t)cap, *h_sup = h_pop + cap;
  nemo::HostCopies hc;
  hc.add(h_hash, a.hash, 16ull * nu);
  hc.add(h_pop, a.pop, 4ull * nu);
  hc.add(h_sup, a.support, 4ull * V0);
  nemo::launch_to_host_multi(hc, s);
  HIPCHK(c, hipEventRecord(c->ev_dclass, s));
  HIPCHK(c, hipEventSynchronize(c->ev_dclass));
  std::vector<dclass::Hash> hash(nu);
  for (uint32_t u = 0; u < nu; u++) memcpy(&hash[u], h_hash + 4 * (size_t)u, 16);
  std::vector<uint32_t> pop(h_pop, h_pop + nu);
  cs.dc_support.assign(h_sup, h_sup + V0);
  dclass::Refiner ref(hash.data(), nu, c->opt.class_hash_bits);
  std::vector<uint32_t> pairs;
  uint8_t *h_v = reinterpret_cast<uint8_t *>(c->h_dcout.p);
  while (ref.next_round(pairs)) {
    const uint32_t np = (uint32_t)(pairs.size() / 2);  // < nu
    if (np) {
      memcpy(c->h_dcin.p, pairs.data(), pairs.size() * 4);
      nemo::launch_to_host(cs.d_dcin.p, c->h_dcin.p, 8ull * np, s);
      // each verified row and its candidate once more
      if ((rc = timed_on(c, s, "k_dclass", 2.0 * np * V0 + 9.0 * np, 0,
                         [&] { nemo::launch_dclass_cmp(a, cs.d_dcin.p, np, cs.d_dcv.p, s); })))
        return rc;
      nemo::launch_to_host(h_v, cs.d_dcv.p, np, s);
      HIPCHK(c, hipEventRecord(c->ev_dclass, s));
      HIPCHK(c, hipEventSynchronize(c->ev_dclass));
    }
    ref.verdicts(h_v);
  }
  cs.dc_rounds = ref.rounds();
  dclass::finish(ref.rep(), cs.dmap.data(), n, first.data(), pop.data(), cs.dc_class_of, cs.dc_classes);
  for (uint32_t u = 0; u < nu; u++)
    if (ref.rep()[u] == u) cs.dc_hash.push_back(hash[u]);
  cs.dc_done = true;
  return NEMO_OK;
}

int nemo_fetch_diff_classes(nemo_ctx *c, uint32_t *class_of, nemo_diff_class *classes, uint64_t cap, uint64_t *n_classes) {
  DISPATCH(node_fetch_diff_classes(c, class_of, classes, cap, n_classes));
  // no ensure_whole: reads the host results of nemo_diff_classes, no graph
  if (!c) return NEMO_ERR_INVALID;
  if (!c->cs.dc_done) return fail(c, NEMO_ERR_STATE, "nemo_fetch_diff_classes before nemo_diff_classes (or after a later nemo_diffprov)");
  const uint64_t k = c->cs.dc_classes.size();
  if (n_classes) *n_classes = k;
  if (class_of && !c->cs.dc_class_of.empty()) memcpy(class_of, c->cs.dc_class_of.data(), c->cs.dc_class_of.size() * 4);
  if (!classes) return NEMO_OK;
  if (cap < k) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  if (k) memcpy(classes, c->cs.dc_classes.data(), k * sizeof(nemo_diff_class));
  return NEMO_OK;
}

int nemo_fetch_diff_support(nemo_ctx *c, uint32_t *out, uint64_t cap) {
  DISPATCH(node_fetch_diff_support(c, out, cap));
  // no ensure_whole: reads the host results of nemo_diff_classes, no graph
  if (!c) return NEMO_ERR_INVALID;
  if (!c->cs.dc_done) return fail(c, NEMO_ERR_STATE, "nemo_fetch_diff_support before nemo_diff_classes (or after a later nemo_diffprov)");
  const uint64_t V0 = c->cs.dc_support.size();
  if (V0 && !out) return NEMO_ERR_INVALID;
  if (cap < V0) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  if (V0) memcpy(out, c->cs.dc_support.data(), V0 * 4);
  return NEMO_OK;
}

// ---- symmetric differential provenance ("bad - good"; DESIGN.md §Symmetric diff) ----
// Entry e walks its own graph (failed run e's raw post graph) against run 0's
// post-goal label hash: one launch over all entries, on the context's stream,
// in call order.  Results stay in HBM until fetched; the state is disjoint
// from nemo_diffprov's.
//
// nemo_diffprov_pairs (DESIGN.md §Pair diff) is the same body with the run compared against
// chosen per entry (`other_iters`, null for the symmetric call): entry e walks base run e's post
// graph against the label hash of other run e.  An entry against run 0 probes the load's table as
// the symmetric call does; k_lab_hash builds a table for every other distinct `other` run in the
// per-call region d_phreg, on the context's stream ahead of the walk.
static int sdiff_impl(nemo_ctx *c, bool per_pair, const uint32_t *failed_iters, const uint32_t *other_iters,
                      size_t n_failed) {
  const char *who = per_pair ? "nemo_diffprov_pairs" : "nemo_diffprov_symmetric";
  if (c && c->node)
    return fail(c, NEMO_ERR_STATE, "%s: single-device contexts only (a node context does not fan it out)", who);
  if (!c || ((!failed_iters || (per_pair && !other_iters)) && n_failed)) return NEMO_ERR_INVALID;
  if (!c->cs.loaded) return fail(c, NEMO_ERR_STATE, "%s without a loaded corpus (the last load failed?)", who);
  if (!c->cs.marked) return fail(c, NEMO_ERR_STATE, "%s before nemo_mark_holds", who);
  HIPCHK(c, hipSetDevice(c->device));
  if (int rw = ensure_whole(c)) return rw;  // may read any graph
  c->cs.n_sentries = 0;
  c->cs.sd_done = false;
  c->cs.sd_graph.clear();
  c->cs.sd_off.assign(1, 0);
  // nothing to compare (with): zero entries, as nemo_diffprov; the pairs call names its own `other` runs
  if (n_failed == 0 || (!per_pair && c->cs.run0 < 0)) {
    c->cs.sd_done = true;
    return NEMO_OK;
  }
  if (n_failed > 0xFFFFFFFFull) return fail(c, NEMO_ERR_LIMIT, "too many diff entries");
  std::vector<uint32_t> graph(n_failed), other;
  std::vector<uint64_t> off(n_failed + 1, 0);
  uint32_t n_lds = 0, n_glob = 0;
  // algorithmic bytes per entry: rows both ways (8E + 8V), node word + label + Kahn order (12V),
  // the mask written (V); the three sweeps are counted as traversed edges
  double bytes = 0, edges = 0;
  int rc;
  if (per_pair) other.resize(n_failed);
  for (size_t e = 0; e < n_failed; e++) {
    uint32_t r;
    if (per_pair) {
      if ((rc = run_index(c, other_iters[e], &r))) return rc;
      other[e] = 2 * r + 1;
    }
    if ((rc = run_index(c, failed_iters[e], &r))) return rc;
    const uint32_t g = 2 * r + 1;
    const uint64_t V = c->cs.nv(g), E = c->cs.ne(g);
    graph[e] = g;
    off[e + 1] = off[e] + V;
    if (tier_fits(c->cs.dc.t_diff, (uint32_t)std::min<uint64_t>(V, ~0u), (uint32_t)std::min<uint64_t>(E, ~0u), 0)) n_lds++;
    else n_glob++;
    bytes += 8.0 * E + 21.0 * V;
    edges += 3.0 * E;
  }
  const uint64_t total = off[n_failed];
  CorpusState &cs = c->cs;
  // the pairs call's tables (pairs_host.h): one per distinct `other` run but run 0, whose table the load built
  pairs::Plan plan;
  if (per_pair) {
    plan = pairs::plan(other.data(), n_failed, cs.node_off.data(), cs.run0 >= 0 ? (int64_t)cs.g0() : -1);
    if (!plan.ok) return fail(c, NEMO_ERR_LIMIT, "%s: a label table would exceed 2^32 slots", who);
  }
  const size_t n_tabs = plan.tab_graph.size();
  // per-entry buffers in whole 64-entry chunks; the ragged ones and the table region exactly the largest request so far
  const uint64_t ecap = (n_failed + 63) & ~(uint64_t)63;
  const bool grow_e = ecap > cs.d_sdgraph.cap || !cs.d_sdoff.p, grow_v = total > cs.d_sdmask.cap || !cs.d_sdrows.p;
  if (grow_e || grow_v || (per_pair && 2 * ecap > cs.d_sdtab.cap) || plan.words > cs.d_phreg.cap || (n_glob && !cs.d_sdbits.p)) {
    // an earlier symmetric / pairs call or its pull may still use the buffers
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // entry descriptors, then table descriptors (at most one per entry)
    if (per_pair && (rc = cs.d_sdtab.grow(c, 2 * ecap))) return rc;
    if (plan.words && (rc = cs.d_phreg.grow(c, plan.words))) return rc;
    if (grow_e) {
      cs.d_sdgraph.release(c), cs.d_sdoff.release(c);
      if ((rc = cs.d_sdgraph.grow(c, ecap)) || (rc = cs.d_sdoff.grow(c, ecap + 1))) return rc;
    }
    if (grow_v) {
      cs.d_sdmask.release(c), cs.d_sddepth.release(c), cs.d_sdrows.release(c), cs.d_sdbits.release(c);
      // a row per S rule at most, and the rules of all entries are at most their nodes: no overflow
      if ((rc = cs.d_sdmask.grow(c, total)) || (rc = cs.d_sddepth.grow(c, total)) || (rc = cs.d_sdrows.grow(c, 2 * total + 2)))
        return rc;
    }
    // node bits of the global tier only, as many as d_sdmask holds (live ones were allocated at that size)
    if (n_glob && (rc = cs.d_sdbits.grow(c, cs.d_sdmask.cap))) return rc;
  }
  if ((rc = cs.d_sdn.grow(c, 1))) return rc;
  hipStream_t s = c->stream;
  HIPCHK(c, hipMemcpyAsync(c->cs.d_sdgraph.p, graph.data(), n_failed * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->cs.d_sdoff.p, off.data(), (n_failed + 1) * 8, hipMemcpyHostToDevice, s));
  nemo::launch_zero(c->cs.d_sdn.p, 4, s);
  std::vector<nemo::LabTab> tabs;  // (kept in sd_tabs below, as graph and off are: the uploads read them)
  if (per_pair) {
    // [entries] the table each entry probes, then [tables] the tables k_lab_hash fills
    tabs.resize(n_failed + n_tabs);
    for (size_t t = 0; t < n_tabs; t++)
      tabs[n_failed + t] = {c->cs.d_phreg.p + plan.tab_off[t], plan.tab_mask[t], plan.tab_graph[t]};
    for (size_t e = 0; e < n_failed; e++)
      tabs[e] = plan.entry_tab[e] == PAIRS_SHARED ? nemo::LabTab{c->cs.d_r0hkey, c->cs.r0hmask, other[e]}
                                                   : tabs[n_failed + plan.entry_tab[e]];
    HIPCHK(c, hipMemcpyAsync(c->cs.d_sdtab.p, tabs.data(), tabs.size() * sizeof(nemo::LabTab), hipMemcpyHostToDevice, s));
    // tables of at most pair_hash_lds_max slots are built in LDS; the launch's LDS is the largest of them
    const uint32_t lds_max = c->opt.pair_hash_lds_max;
    uint32_t lds_slots = 0;
    for (size_t t = 0; t < n_tabs; t++)
      if (plan.tab_mask[t] < lds_max) lds_slots = std::max(lds_slots, plan.tab_mask[t] + 1u);
    // algorithmic bytes: node word + label of every hashed graph, and the tables written
    if (n_tabs && (rc = timed(c, "k_lab_hash", 8.0 * (double)plan.nodes + 4.0 * (double)plan.words, 0, [&] {
           nemo::launch_lab_hash(c->cs.dc, c->cs.d_sdtab.p + n_failed, (uint32_t)n_tabs, lds_max, lds_slots, s);
         })))
      return rc;
  }
  nemo::SdiffArgs a{};
  a.graph = c->cs.d_sdgraph.p;
  a.off = c->cs.d_sdoff.p;
  a.r0hkey = c->cs.d_r0hkey;
  a.r0hmask = c->cs.r0hmask;
  a.tabs = per_pair ? c->cs.d_sdtab.p : nullptr;
  a.bits = c->cs.d_sdbits.p;
  a.depth = c->cs.d_sddepth.p;
  a.mask = c->cs.d_sdmask.p;
  a.rows = c->cs.d_sdrows.p;
  a.n_rows = c->cs.d_sdn.p;
  if ((rc = timed(c, "k_sdiff", bytes, edges,
                  [&] { nemo::launch_sdiff(c->cs.dc, a, (uint32_t)n_failed, n_lds, n_glob, s); })))
    return rc;
  c->cs.sd_graph = std::move(graph);
  c->cs.sd_off = std::move(off);
  c->cs.sd_tabs = std::move(tabs);
  c->cs.n_sentries = (uint32_t)n_failed;
  c->cs.sd_done = true;
  return NEMO_OK;
}

int nemo_diffprov_symmetric(nemo_ctx *c, const uint32_t *failed_iters, size_t n_failed) {
  return sdiff_impl(c, false, failed_iters, nullptr, n_failed);
}

int nemo_diffprov_pairs(nemo_ctx *c, const uint32_t *base_iters, const uint32_t *other_iters, size_t n) {
  return sdiff_impl(c, true, base_iters, other_iters, n);
}

int nemo_fetch_sdiff_masks(nemo_ctx *c, uint64_t *off, uint8_t *out, uint64_t cap, uint64_t *n_used) {
  if (!c) return NEMO_ERR_INVALID;
  if (!c->cs.sd_done) return fail(c, NEMO_ERR_STATE, "nemo_fetch_sdiff_masks before nemo_diffprov_symmetric");
  const uint64_t total = c->cs.sd_off.back();
  if (n_used) *n_used = total;
  if (off) memcpy(off, c->cs.sd_off.data(), c->cs.sd_off.size() * 8);
  if (!out) return NEMO_OK;
  if (cap < total) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  if (total) {
    HIPCHK(c, hipSetDevice(c->device));
  if (int rw = ensure_whole(c)) return rw;  // may read any graph
    HIPCHK(c, hipMemcpyAsync(out, c->cs.d_sdmask.p, total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return NEMO_OK;
}

int nemo_fetch_surplus(nemo_ctx *c, nemo_missing *out, uint64_t cap, uint64_t *n_out) {
  if (!c) return NEMO_ERR_INVALID;
  if (!c->cs.sd_done) return fail(c, NEMO_ERR_STATE, "nemo_fetch_surplus before nemo_diffprov_symmetric");
  uint32_t n = 0;
  if (c->cs.n_sentries) {
    HIPCHK(c, hipSetDevice(c->device));
  if (int rw = ensure_whole(c)) return rw;  // may read any graph
    HIPCHK(c, hipMemcpyAsync(&n, c->cs.d_sdn.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (n_out) *n_out = n;
  if (!out) return NEMO_OK;
  if (cap < n) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  if (!n) return NEMO_OK;
  std::vector<uint32_t> rows(2 * (size_t)n);
  HIPCHK(c, hipMemcpyAsync(rows.data(), c->cs.d_sdrows.p, 8ull * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  sort_rows<2>(rows.data(), n);  // the device emits in any order: by (entry, rule)
  for (uint32_t k = 0; k < n; k++) {
    out[k].entry = rows[2 * k];
    out[k].rule = rows[2 * k + 1];
  }
  return NEMO_OK;
}

}  // extern "C"
