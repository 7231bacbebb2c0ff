// repair_api.h — the absent-set front end the four repair calls share (api_repair.hip: nemo_min_repair_sets,
// nemo_min_repairs; api_lrepair.hip: nemo_lineage_repair_sets, nemo_lineage_repairs; DESIGN.md §Minimal repair sets,
// §Lineage repair search): the explicit form's list checks with their messages and its bitmap and candidates on their
// way to the device, and the pair form's device-made absent set.  The state is the calling family's (ctx.h: its
// AbsentSet, candidate buffer, pinned buffer and event, handed in); nothing here owns any, and neither family's calls
// touch the other's.  The callers keep their entry checks, their limits and early ends, and their timing group, which
// they open between the checks and the queue.  The arithmetic is repair_host.h's and pairs_host.h's.
#pragma once
#include "knock_api.h"

// The explicit form's two lists against a graph of V nodes (repair::check_lists), with the calls' messages.
static inline int absent_check(nemo_ctx *c, const char *who, const uint32_t *absent, size_t n_absent, const uint32_t *cand, size_t n_cand,
                               uint64_t V) {
  size_t where = 0;
  switch (repair::check_lists(absent, n_absent, cand, n_cand, V, &where)) {
    case repair::ABSENT_RANGE:
      return fail(c, NEMO_ERR_INVALID, "%s: absent node %zu is node %u, out of range (%llu nodes)", who, where, absent[where],
                  (unsigned long long)V);
    case repair::ABSENT_DUP:
      return fail(c, NEMO_ERR_INVALID, "%s: absent node %zu names node %u a second time", who, where, absent[where]);
    case repair::CAND_DUP:
      return fail(c, NEMO_ERR_INVALID, "%s: candidate %zu names node %u a second time", who, where, cand[where]);
    case repair::CAND_NOT_ABSENT:
      return fail(c, NEMO_ERR_INVALID, "%s: candidate %zu is node %u, which is not in the absent list", who, where, cand[where]);
    default:
      return NEMO_OK;
  }
}

// The explicit form, its lists checked: the bitmap of absent[n_absent] over graph g built and queued into st.d_bits,
// the candidates h_cand queued into d_cand, and *L = the graph's Kahn level count, for the tier.  h / ev: the
// family's pinned buffer (8 elements at least) and event.
template <class T>
static int absent_queue(nemo_ctx *c, AbsentSet &st, DevBuf<uint32_t> &d_cand, const std::vector<uint32_t> &h_cand, Pinned<T> &h, hipEvent_t ev,
                        uint32_t g, const uint32_t *absent, size_t n_absent, uint32_t *L) {
  CorpusState &cs = c->cs;
  hipStream_t s = c->stream;
  const uint64_t V = cs.nv(g), K = h_cand.size();
  int rc;
  {
    const uint64_t need[2] = {repair::bitmap_words(V), std::max<uint64_t>(K, 1)};
    if ((rc = grow_group(c, need, st.d_bits, d_cand))) return rc;
  }
  st.bits = repair::bitmap(absent, n_absent, V);
  HIPCHK(c, hipMemcpyAsync(st.d_bits.p, st.bits.data(), 8 * st.bits.size(), hipMemcpyHostToDevice, s));
  if (K) HIPCHK(c, hipMemcpyAsync(d_cand.p, h_cand.data(), 4 * K, hipMemcpyHostToDevice, s));
  nemo::launch_to_host(h.p, cs.dc.nlev + g, 4, s);
  if ((rc = wait_copied(c, ev))) return rc;
  *L = reinterpret_cast<const uint32_t *>(h.p)[0];
  return NEMO_OK;
}

// The pair form: A = cand = the sink goals of graph g (base's post graph) whose label is no goal label of graph go
// (other's post graph), made on the device into st.d_bits and d_cand.  The other run's table is the load's for run 0,
// else k_lab_hash's in st.d_hreg, as nemo_diffprov_pairs'.  *bytes: what the launches move, added; *K, *L: the absent
// sink goals beside the graph's Kahn level count, read in one copy.
template <class T>
static int absent_pair(nemo_ctx *c, const char *who, AbsentSet &st, DevBuf<uint32_t> &d_cand, Pinned<T> &h, hipEvent_t ev, uint32_t g,
                       uint32_t go, double *bytes, uint64_t *K, uint32_t *L) {
  CorpusState &cs = c->cs;
  hipStream_t s = c->stream;
  const uint64_t V = cs.nv(g);
  int rc;
  const pairs::Plan plan = pairs::plan(&go, 1, cs.node_off.data(), cs.run0 >= 0 ? (int64_t)cs.g0() : -1);
  if (!plan.ok) return fail(c, NEMO_ERR_LIMIT, "%s: a label table would exceed 2^32 slots", who);
  const bool shared = plan.entry_tab[0] == PAIRS_SHARED;
  if (!st.d_cnt.p || (!shared && (!st.d_tab.p || plan.words > st.d_hreg.cap || !st.d_hreg.p))) {
    HIPCHK(c, hipStreamSynchronize(s));  // an earlier call may still use them
    if ((rc = st.d_cnt.grow(c, 2))) return rc;
    if (!shared && ((rc = st.d_tab.grow(c, 1)) || (rc = st.d_hreg.grow(c, plan.words)))) return rc;
  }
  {
    const uint64_t need[2] = {repair::bitmap_words(V), V};
    if ((rc = grow_group(c, need, st.d_bits, d_cand))) return rc;
  }
  st.tab = shared ? nemo::LabTab{cs.d_r0hkey, cs.r0hmask, go} : nemo::LabTab{st.d_hreg.p, plan.tab_mask[0], go};
  if (!shared) {
    HIPCHK(c, hipMemcpyAsync(st.d_tab.p, &st.tab, sizeof(nemo::LabTab), hipMemcpyHostToDevice, s));
    const uint32_t lds_max = c->opt.pair_hash_lds_max;
    const uint32_t lds_slots = plan.tab_mask[0] < lds_max ? plan.tab_mask[0] + 1u : 0u;
    const double b = 8.0 * (double)plan.nodes + 4.0 * (double)plan.words;
    if ((rc = timed(c, "k_lab_hash", b, 0, [&] { nemo::launch_lab_hash(cs.dc, st.d_tab.p, 1, lds_max, lds_slots, s); }))) return rc;
    *bytes += b;
  }
  {
    // node word, label and two row pointers of every node, a probe per sink goal, the bitmap and the list written
    const double b = 20.0 * (double)V + (double)V / 8.0 + 8.0;
    if ((rc = timed(c, "k_repair_absent", b, 0,
                    [&] { nemo::launch_repair_absent(cs.dc, g, st.tab.key, st.tab.mask, st.d_bits.p, d_cand.p, st.d_cnt.p, s); })))
      return rc;
    *bytes += b;
  }
  nemo::launch_to_host(h.p, st.d_cnt.p, 8, s);  // the count beside the Kahn level count
  if ((rc = wait_copied(c, ev))) return rc;
  *K = reinterpret_cast<const uint32_t *>(h.p)[0];
  *L = reinterpret_cast<const uint32_t *>(h.p)[1];
  return NEMO_OK;
}
