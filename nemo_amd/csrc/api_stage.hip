// api_stage.hip — triggers, chain and node-flag fetches, and the staged hand-over of the simplification.
#include "ctx.h"

extern "C" {

int nemo_triggers(nemo_ctx *c) {
  DISPATCH(node_triggers(c));
  if (!c) return NEMO_ERR_INVALID;
  if (!c->cs.marked) return fail(c, NEMO_ERR_STATE, "nemo_triggers before nemo_mark_holds");
  if (int rm = ensure_marked(c)) return rm;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rw = ensure_run0(c)) return rw;  // reads the build outputs of run 0's graphs only
  c->cs.tcounts[0] = c->cs.tcounts[1] = c->cs.tcounts[2] = 0;
  c->cs.trig_done = true;
  c->cs.trig_pending = false;
  if (c->cs.run0 < 0) return NEMO_OK;
  int rc;
  if ((rc = c->cs.d_tcounts.grow(c, 3))) return rc;
  if ((rc = c->h_tcounts.grow(c, 4))) return rc;
  if ((rc = ensure_event(c, &c->ev_trig))) return rc;
  nemo::TrigArgs a{};
  a.g_pre = 2 * c->cs.run0;
  a.g_post = c->cs.g0();
  a.counts = c->cs.d_tcounts.p;
  a.pre = c->cs.d_tpre;
  a.post = c->cs.d_tpost;
  a.async_rules = c->cs.d_tasync;
  hipStream_t s = c->stream;
  nemo::launch_zero(c->cs.d_tcounts.p, 12, s);
  rc = timed(c, "k_triggers", 0, 0, [&] { nemo::launch_triggers(c->cs.dc, a, 1, s); });
  if (rc) return rc;
  if ((rc = c->h_tpre.grow(c, 3 * c->cs.tcap[0] + 3))) return rc;
  if ((rc = c->h_tpost.grow(c, 2 * c->cs.tcap[1] + 2))) return rc;
  if ((rc = c->h_tasync.grow(c, c->cs.tcap[2] + 1))) return rc;
  nemo::HostCopies hc;
  hc.add(c->h_tcounts.p, c->cs.d_tcounts.p, 12);
  hc.add(c->h_tpre.p, c->cs.d_tpre, 12 * c->cs.tcap[0]);
  hc.add(c->h_tpost.p, c->cs.d_tpost, 8 * c->cs.tcap[1]);
  hc.add(c->h_tasync.p, c->cs.d_tasync, 4 * c->cs.tcap[2]);
  nemo::launch_to_host_multi(hc, s);
  HIPCHK(c, hipEventRecord(c->ev_trig, s));
  c->cs.trig_pending = true;
  return NEMO_OK;
}

static int trig_sync(nemo_ctx *c) {
  if (!c->cs.trig_pending) return NEMO_OK;
  HIPCHK(c, hipEventSynchronize(c->ev_trig));
  for (int i = 0; i < 3; i++) {
    if (c->h_tcounts.p[i] > c->cs.tcap[i]) return fail(c, NEMO_ERR_LIMIT, "trigger rows exceed their bound");
    c->cs.tcounts[i] = c->h_tcounts.p[i];
  }
  c->cs.trig_pending = false;
  return NEMO_OK;
}

int nemo_fetch_triggers(nemo_ctx *c, uint32_t *pre, uint64_t pre_cap, uint64_t *n_pre, uint32_t *post,
                        uint64_t post_cap, uint64_t *n_post, uint32_t *async_rules, uint64_t async_cap,
                        uint64_t *n_async) {
  DISPATCH(node_fetch_triggers(c, pre, pre_cap, n_pre, post, post_cap, n_post, async_rules, async_cap, n_async));
  if (!c) return NEMO_ERR_INVALID;
  if (!c->cs.trig_done) return fail(c, NEMO_ERR_STATE, "nemo_fetch_triggers before nemo_triggers");
  HIPCHK(c, hipSetDevice(c->device));
  if (int rw = ensure_run0(c)) return rw;  // reads the build outputs of run 0's graphs only
  if (int rt = trig_sync(c)) return rt;
  if (n_pre) *n_pre = c->cs.tcounts[0];
  if (n_post) *n_post = c->cs.tcounts[1];
  if (n_async) *n_async = c->cs.tcounts[2];
  if (pre && c->cs.tcounts[0]) {
    if (pre_cap < c->cs.tcounts[0]) return fail(c, NEMO_ERR_INVALID, "capacity too small");
    memcpy(pre, c->h_tpre.p, 12 * (size_t)c->cs.tcounts[0]);
  }
  if (post && c->cs.tcounts[1]) {
    if (post_cap < c->cs.tcounts[1]) return fail(c, NEMO_ERR_INVALID, "capacity too small");
    memcpy(post, c->h_tpost.p, 8 * (size_t)c->cs.tcounts[1]);
  }
  if (async_rules && c->cs.tcounts[2]) {
    if (async_cap < c->cs.tcounts[2]) return fail(c, NEMO_ERR_INVALID, "capacity too small");
    memcpy(async_rules, c->h_tasync.p, 4 * (size_t)c->cs.tcounts[2]);
  }
  if (pre) sort_rows<3>(pre, c->cs.tcounts[0]);
  if (post) sort_rows<2>(post, c->cs.tcounts[1]);
  if (async_rules) std::sort(async_rules, async_rules + c->cs.tcounts[2]);
  return NEMO_OK;
}

int nemo_fetch_node_flags(nemo_ctx *c, uint32_t g_lo, uint32_t g_hi, uint8_t *out, uint64_t cap) {
  DISPATCH(node_fetch_node_flags(c, g_lo, g_hi, out, cap));
  if (!c || !out || g_lo > g_hi || g_hi > c->cs.G) return NEMO_ERR_INVALID;
  if (!c->cs.marked) return fail(c, NEMO_ERR_STATE, "no flags before nemo_mark_holds");
  const uint64_t a = c->cs.node_off[g_lo], b = c->cs.node_off[g_hi];
  if (cap < b - a) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  HIPCHK(c, hipSetDevice(c->device));
  if (int rw = ensure_whole(c)) return rw;  // may read any graph
  if (int rm = ensure_marked(c)) return rm;
  if (b > a) {
    HIPCHK(c, hipMemcpyAsync(out, c->cs.dc.flags + a, b - a, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return NEMO_OK;
}

int nemo_fetch_chains(nemo_ctx *c, nemo_chain *out, uint64_t cap, uint64_t *n_out) {
  DISPATCH(node_fetch_chains(c, out, cap, n_out));
  if (!c) return NEMO_ERR_INVALID;
  if (!c->cs.simplified) return fail(c, NEMO_ERR_STATE, "no chains before nemo_simplify");
  HIPCHK(c, hipSetDevice(c->device));
  if (int rw = ensure_whole(c)) return rw;  // may read any graph
  int rc;
  hipStream_t s = c->stream;
  if ((rc = c->cs.d_choff.grow(c, (uint64_t)c->cs.G + 1))) return rc;
  rc = timed(c, "k_chain_gather", 0, 0, [&] { nemo::launch_chain_gather(c->cs.dc, c->cs.d_choff.p, nullptr, s); });
  if (rc) return rc;
  uint64_t n = 0;
  HIPCHK(c, hipMemcpyAsync(&n, c->cs.d_choff.p + c->cs.G, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  if (n_out) *n_out = n;
  if (!out) return NEMO_OK;
  if (cap < n) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  if (5 * n > c->cs.d_chout.cap && (rc = c->cs.d_chout.grow(c, 5 * n))) return rc;
  rc = timed(c, "k_chain_gather", 0, 0, [&] { nemo::launch_chain_gather(c->cs.dc, c->cs.d_choff.p, c->cs.d_chout.p, s); });
  if (rc) return rc;
  static_assert(sizeof(nemo_chain) == 20, "nemo_chain layout");
  if (n) HIPCHK(c, hipMemcpyAsync(out, c->cs.d_chout.p, n * 20, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return NEMO_OK;
}

// bulk D2H on the copy stream: the runtime's copies (SDMA if asked, else its blit kernel on the
// copy stream's CUs) or a k_to_host grid of stage_blocks workgroups
static hipError_t stage_copy(nemo_ctx *c, void *dst, const void *src, size_t n) {
  if (!n) return hipSuccess;
  if (c->opt.stage_blocks) {
    nemo::launch_to_host(dst, src, n, c->copy, c->opt.stage_blocks);
    return hipGetLastError();
  }
  if (c->opt.stage_sdma) {
    if (hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDeviceNoCU, c->copy) == hipSuccess) return hipSuccess;
    (void)hipGetLastError();
    c->opt.stage_sdma = false;
  }
  return hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, c->copy);
}

// The 2-bit node state on stream s and its copy, in K slices of whole words, each stage_ratio times the
// one before; s has reached the point where the flags are final.  Each slice's copy waits for that
// slice's k_pack_state only, so the link starts behind the first, short slice; an empty slice (fewer
// words than slices) issues nothing, but the last.
static int stage_state(nemo_ctx *c, hipStream_t s, uint32_t K) {
  int rc;
  const uint64_t words = stage::state_words(c->cs.V), sbytes = 4 * words;  // 2-bit node state
  if ((rc = c->cs.d_state.grow(c, sbytes / 4 + 1))) return rc;
  if ((rc = c->h_flags.grow(c, sbytes + 16))) return rc;
  for (uint32_t k = 0; k < K; k++) {
    const stage::Range w = stage::slice(words, K, k, c->opt.stage_ratio);
    if (w.empty() && k + 1 < K) continue;
    rc = timed_on(c, s, "k_pack_state", (double)stage::state_nodes(c->cs.V, w) + 4.0 * (double)w.size(), 0,
                  [&] { nemo::launch_pack_state(c->cs.dc.flags, c->cs.d_state.p, c->cs.V, w.lo, w.size(), s); });
    if (rc) return rc;
    if ((rc = ensure_event(c, &c->ev_state[k]))) return rc;
    HIPCHK(c, hipEventRecord(c->ev_state[k], s));
    HIPCHK(c, hipStreamWaitEvent(c->copy, c->ev_state[k], 0));
    HIPCHK(c, stage_copy(c, c->h_flags.p + 4 * w.lo, c->cs.d_state.p + w.lo, 4 * w.size()));
  }
  return NEMO_OK;
}

// Enqueue the chain pairs at a capacity of `cap` pairs, in K slices of the pair indices, and their bulk
// copies on the copy stream (behind the node state's, which stage_state queued first).  Each slice's
// copy waits for that slice's k_chain_pairs only; the offsets' copy and ev_copied follow the last slice,
// which is issued even when it is empty.
static int stage_enqueue(nemo_ctx *c, uint64_t cap, uint32_t K) {
  int rc;
  hipStream_t s = c->cs.stage_stream ? c->cs.stage_stream : c->stream;
  const uint64_t pw = c->cs.pairs_wide ? 2 : 1;  // u32 words per pair
  if (pw * cap + 2 > c->cs.d_chht.cap) {
    HIPCHK(c, hipStreamSynchronize(s));
    if ((rc = c->cs.d_chht.grow(c, pw * cap + 2))) return rc;
  }
  if ((rc = c->h_chht.grow(c, pw * cap + 2))) return rc;
  for (uint32_t k = 0; k < K; k++) {
    const stage::Range r = stage::slice(cap, K, k);
    const bool last = k + 1 == K;
    if (r.empty() && !last) continue;
    rc = timed_on(c, s, "k_chain_pairs", 4.0 * pw * (double)r.size() + (last ? 20.0 * c->cs.G : 0.0), 0, [&] {
      nemo::launch_chain_pairs(c->cs.dc, c->cs.d_choff.p, c->cs.d_chht.p, r.lo, r.hi, c->cs.pairs_wide ? 1 : 0, s);
    });
    if (rc) return rc;
    if (last) nemo::launch_to_host(c->h_choff.p, c->cs.d_choff.p, ((size_t)c->cs.G + 1) * 8, s);
    if ((rc = ensure_event(c, &c->ev_ready[k]))) return rc;
    HIPCHK(c, hipEventRecord(c->ev_ready[k], s));
    HIPCHK(c, hipStreamWaitEvent(c->copy, c->ev_ready[k], 0));
    HIPCHK(c, stage_copy(c, c->h_chht.p + pw * r.lo, c->cs.d_chht.p + pw * r.lo, pw * r.size() * 4));
  }
  HIPCHK(c, hipEventRecord(c->ev_copied, c->copy));
  c->cs.staged_cap = cap;
  return NEMO_OK;
}

int nemo_stage_simplified(nemo_ctx *c) {
  DISPATCH(node_stage_simplified(c));
  if (!c) return NEMO_ERR_INVALID;
  if (!c->cs.simplified) return fail(c, NEMO_ERR_STATE, "nemo_stage_simplified before nemo_simplify");
  HIPCHK(c, hipSetDevice(c->device));
  // no ensure_whole: the hand-over kernels read flags, nch and chain, which are replicated behind their kernels
  int rc;
  hipStream_t s = c->stream;
  if (!c->copy) {
    // the bulk D2H copies run as the runtime's blit kernel, PCIe-bound for ~0.5 ms
    // per step: confined to a few CUs, they no longer hold workgroup slots of
    // the LDS-tier kernel running beside them (stage_cus, default 8; 0 = any CU)
    if (c->opt.stage_cus) {
      uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (uint32_t k = 0; k < std::min(c->opt.stage_cus, 256u); k++) mask[k >> 5] |= 1u << (k & 31);
      if (hipExtStreamCreateWithCUMask(&c->copy, 8, mask) != hipSuccess) {
        (void)hipGetLastError();
        c->copy = nullptr;
      }
    }
    if (!c->copy) HIPCHK(c, hipStreamCreateWithFlags(&c->copy, hipStreamNonBlocking));
  }
  if ((rc = ensure_event(c, &c->ev_copied))) return rc;
  const uint32_t K = std::min(std::max(c->opt.stage_slices, 1u), NEMO_STAGE_SLICES_MAX);
  const uint32_t KP = std::min(std::max(c->opt.stage_pair_slices, 1u), NEMO_STAGE_SLICES_MAX);
  if (c->cs.staged) HIPCHK(c, hipEventSynchronize(c->ev_copied));  // host buffers are reused
  c->cs.staged = false;
  if ((rc = c->cs.d_choff.grow(c, (uint64_t)c->cs.G + 1))) return rc;
  if ((rc = c->h_choff.grow(c, (uint64_t)c->cs.G + 1))) return rc;
  if (c->opt.stage_on_aux) {  // read-only on the analysis: `stream` goes on to the triggers and pulls
    if (!c->aux) HIPCHK(c, hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking));
    // the node state from where nemo_simplify's flags were final (beside the chain cover), then
    // the chain pairs from where its chains were (ev_simp: beside whatever the caller queued since)
    if (!c->cs.flags_final) {  // flags rewritten since nemo_simplify: pack them where `stream` is now
      if ((rc = ensure_event(c, &c->ev_flags))) return rc;
      HIPCHK(c, hipEventRecord(c->ev_flags, c->stream));
    }
    HIPCHK(c, hipStreamWaitEvent(c->aux, c->ev_flags, 0));
    if ((rc = stage_state(c, c->aux, K))) return rc;
    if (c->cs.chains_final) {
      HIPCHK(c, hipStreamWaitEvent(c->aux, c->ev_simp, 0));
    } else {  // chain or nch may have been rewritten since nemo_simplify: behind everything queued so far
      if ((rc = ensure_event(c, &c->ev_stage))) return rc;
      HIPCHK(c, hipEventRecord(c->ev_stage, c->stream));
      HIPCHK(c, hipStreamWaitEvent(c->aux, c->ev_stage, 0));
    }
    s = c->aux;
  } else if ((rc = stage_state(c, s, K))) {
    return rc;
  }
  c->cs.stage_stream = s;
  rc = timed_on(c, s, "k_chain_gather", 0, 0, [&] { nemo::launch_chain_gather(c->cs.dc, c->cs.d_choff.p, nullptr, s); });
  if (rc) return rc;
  // the pair count is only known on the device: stage at the last count seen
  // (no host round trip); nemo_simplified_view re-stages if it was too small
  uint64_t cap = c->cs.chht_hint;
  const bool counted = !cap;  // the first stage after a load: the count comes back first, one slice
  if (!cap) {
    if ((rc = ensure_event(c, &c->ev_misc))) return rc;
    nemo::launch_to_host(c->h_choff.p, c->cs.d_choff.p, ((size_t)c->cs.G + 1) * 8, s);
    HIPCHK(c, hipEventRecord(c->ev_misc, s));
    HIPCHK(c, hipEventSynchronize(c->ev_misc));
    cap = c->h_choff.p[c->cs.G];
  }
  if ((rc = stage_enqueue(c, cap, counted ? 1u : KP))) return rc;
  c->cs.staged = true;
  return NEMO_OK;
}

int nemo_simplified_view(nemo_ctx *c, const uint8_t **state, const uint64_t **chain_off, const uint32_t **chain_ht,
                         uint64_t *n_chains, int *wide_pairs) {
  DISPATCH(node_simplified_view(c, state, chain_off, chain_ht, n_chains, wide_pairs));
  if (!c) return NEMO_ERR_INVALID;
  if (!c->cs.staged) return fail(c, NEMO_ERR_STATE, "nothing staged: call nemo_stage_simplified");
  HIPCHK(c, hipSetDevice(c->device));
  // no ensure_whole: reads the staged flags and chain pairs, no build output
  HIPCHK(c, hipEventSynchronize(c->ev_copied));
  const uint64_t n = c->h_choff.p[c->cs.G];
  if (n > c->cs.staged_cap) {  // the hint was short: stage again at the real count
    // on the context's stream, behind everything queued since the first stage (work that
    // rewrites flags may follow it there; `aux` was ordered only after the first stage)
    c->cs.stage_stream = c->stream;
    int rc = stage_enqueue(c, n, 1);
    if (rc) return rc;
    HIPCHK(c, hipEventSynchronize(c->ev_copied));
  }
  c->cs.chht_hint = n;
  c->cs.staged_n = n;
  if (state) *state = c->h_flags.p;
  if (wide_pairs) *wide_pairs = c->cs.pairs_wide ? 1 : 0;
  if (chain_off) *chain_off = c->h_choff.p;
  if (chain_ht) *chain_ht = c->h_chht.p;
  if (n_chains) *n_chains = c->cs.staged_n;
  return NEMO_OK;
}

}  // extern "C"
