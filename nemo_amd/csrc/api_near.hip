// api_near.hip — nemo_nearest_runs and its fetches (k_near.hip; DESIGN.md §Nearest runs).
#include "ctx.h"

extern "C" {

// The post-goal label sets of the runs the two lists name become bit rows (k_near_bits), the
// intersection counts of every (query, candidate) pair a popcount-AND GEMM over them (k_near_isect),
// and k_near_pick turns the counts into distances and picks each query's nearest candidate.  All of it
// on the context's stream; the call ends with the rows in pinned memory.  The state is the call's own:
// no diff state is read or written.
int nemo_nearest_runs(nemo_ctx *c, const uint32_t *query_iters, size_t n_q, const uint32_t *cand_iters, size_t n_c) {
  if (c && c->node)
    return fail(c, NEMO_ERR_STATE, "nemo_nearest_runs: single-device contexts only (a node context does not fan it out)");
  if (!c || (!query_iters && n_q) || (!cand_iters && n_c)) return NEMO_ERR_INVALID;
  CorpusState &cs = c->cs;
  if (!cs.loaded) return fail(c, NEMO_ERR_STATE, "nemo_nearest_runs without a loaded corpus (the last load failed?)");
  cs.near_done = false;
  cs.near_nq = cs.near_nc = 0;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rw = ensure_whole(c)) return rw;  // may read any graph
  int rc;
  if ((rc = ensure_load_checked(c))) return rc;
  std::vector<uint32_t> q_run(n_q), c_run(n_c);
  for (size_t i = 0; i < n_q; i++)
    if ((rc = run_index(c, query_iters[i], &q_run[i]))) return rc;
  for (size_t j = 0; j < n_c; j++)
    if ((rc = run_index(c, cand_iters[j], &c_run[j]))) return rc;
  if (n_q == 0) {  // zero rows
    cs.near_done = true;
    return NEMO_OK;
  }
  if (nearest::check_limits(n_q, n_c, 0, 0) == nearest::LIMIT_PAIRS)
    return fail(c, NEMO_ERR_LIMIT, "nemo_nearest_runs: %zu x %zu pairs exceed 2^30 in one call: tile the queries", n_q, n_c);
  if ((rc = ensure_event(c, &c->ev_near))) return rc;
  if ((rc = c->h_near.grow(c, 4 * (uint64_t)n_q + 4))) return rc;
  hipStream_t s = c->stream;
  // the outer group: every launch of the call between one pair of events
  const bool outer = c->timing && (c->tgroups.empty() || std::find(c->tgroups.begin(), c->tgroups.end(), "k_near") != c->tgroups.end());
  hipEvent_t ta = nullptr;
  if (outer) {
    ta = get_event(c);
    hipEventRecord(ta, s);
  }
  auto give_up = [&](int code) {
    if (ta) c->ev_pool.push_back(ta);
    return code;
  };
  // the largest goal label of the post graphs, once per load
  if (!cs.near_lmax_done) {
    if ((rc = cs.d_nrlmax.grow(c, 1))) return give_up(rc);
    uint64_t vmax = 0;
    for (uint32_t r = 0; r < cs.n_runs; r++) vmax = std::max(vmax, cs.nv(2 * r + 1));
    const uint32_t parts = (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(1, (vmax + 16383) / 16384));
    nemo::launch_zero(cs.d_nrlmax.p, 4, s);
    if ((rc = timed(c, "k_near_lmax", 8.0 * cs.postV, 0, [&] { nemo::launch_near_lmax(cs.dc, parts, cs.d_nrlmax.p, s); })))
      return give_up(rc);
    nemo::launch_to_host(c->h_near.p, cs.d_nrlmax.p, 4, s);
    HIPCHK(c, hipEventRecord(c->ev_near, s));
    HIPCHK(c, hipEventSynchronize(c->ev_near));
    cs.near_lmax = c->h_near.p[0];
    cs.near_lmax_done = true;
  }
  const nearest::Rows rows = nearest::rows(q_run.data(), n_q, c_run.data(), n_c);
  const uint64_t n_rows = rows.run.size(), W = nearest::words_per_row(cs.near_lmax);
  if (nearest::check_limits(n_q, n_c, n_rows, W) != nearest::LIMIT_OK)
    return give_up(fail(c, NEMO_ERR_LIMIT,
                        "nemo_nearest_runs: %llu bit rows of %llu bytes (largest label %u) exceed 2^36 bytes: tile the queries "
                        "(labels are interned ids; sparse ids make long rows)",
                        (unsigned long long)n_rows, (unsigned long long)(8 * W), cs.near_lmax));
  // the five buffers grow as one group, each to the largest request so far, in a fixed order
  const uint64_t need[5] = {n_rows * W, n_rows, (uint64_t)n_q * n_c, 4 * (uint64_t)n_q, n_rows + n_q + n_c};
  if (need[0] > cs.d_nrbits.cap || need[1] > cs.d_nrsize.cap || need[2] > cs.d_nrmat.cap || need[3] > cs.d_nrout.cap ||
      need[4] > cs.d_nrdesc.cap || !cs.d_nrdesc.p) {
    const uint64_t cap[5] = {std::max(need[0], cs.d_nrbits.cap), std::max(need[1], cs.d_nrsize.cap),
                             std::max(need[2], cs.d_nrmat.cap), std::max(need[3], cs.d_nrout.cap),
                             std::max(need[4], cs.d_nrdesc.cap)};
    HIPCHK(c, hipStreamSynchronize(s));  // an earlier call's fetch may still read them
    cs.d_nrbits.release(c), cs.d_nrsize.release(c), cs.d_nrmat.release(c), cs.d_nrout.release(c), cs.d_nrdesc.release(c);
    if ((rc = cs.d_nrbits.grow(c, cap[0])) || (rc = cs.d_nrsize.grow(c, cap[1])) || (rc = cs.d_nrmat.grow(c, cap[2])) ||
        (rc = cs.d_nrout.grow(c, cap[3])) || (rc = cs.d_nrdesc.grow(c, cap[4])))
      return give_up(rc);
  }
  // descriptors: [rows] post graphs, [n_q] query rows, [n_c] candidate rows
  cs.nr_desc.resize(need[4]);
  double nodes = 0;
  for (uint64_t r = 0; r < n_rows; r++) {
    cs.nr_desc[r] = 2 * rows.run[r] + 1;
    nodes += (double)cs.nv(2 * rows.run[r] + 1);
  }
  std::copy(rows.qrow.begin(), rows.qrow.end(), cs.nr_desc.begin() + n_rows);
  std::copy(rows.crow.begin(), rows.crow.end(), cs.nr_desc.begin() + n_rows + n_q);
  HIPCHK(c, hipMemcpyAsync(cs.d_nrdesc.p, cs.nr_desc.data(), need[4] * 4, hipMemcpyHostToDevice, s));
  nemo::NearArgs a{};
  a.row_graph = cs.d_nrdesc.p;
  a.bits = cs.d_nrbits.p;
  a.size = cs.d_nrsize.p;
  a.rows = (uint32_t)n_rows;
  a.W = W;
  a.qrow = cs.d_nrdesc.p + n_rows;
  a.crow = a.qrow + n_q;
  a.n_q = (uint32_t)n_q;
  a.n_c = (uint32_t)n_c;
  a.mat = cs.d_nrmat.p;
  a.out = cs.d_nrout.p;
  // algorithmic bytes: node word + label of every hashed graph and the rows written; every list position's row
  // read once and the matrix written; the op count is the word pairs of the GEMM
  const double b_bits = 8.0 * nodes + 8.0 * (double)(n_rows * W) + 4.0 * (double)n_rows;
  const double b_isect = 8.0 * (double)W * (double)(n_q + n_c), b_mat = 4.0 * (double)n_q * (double)n_c;
  const double ops = (double)n_q * (double)n_c * (double)W;
  if ((rc = timed(c, "k_near_bits", b_bits, 0, [&] { nemo::launch_near_bits(cs.dc, a, c->opt.near_bits_lds_max, s); })))
    return give_up(rc);
  if (n_c) {
    const nearest::Grid g = nearest::grid(n_q, n_c, W, cs.dc.n_cu, c->opt.near_ksplit);
    if (g.ksplit > 1) nemo::launch_zero(a.mat, 4 * (uint64_t)n_q * n_c, s);
    if ((rc = timed(c, "k_near_isect", b_isect + b_mat, ops,
                    [&] { nemo::launch_near_isect(a, g.tq, g.tc, g.slabs, g.slabs_per_split, g.ksplit, s); })))
      return give_up(rc);
  }
  if ((rc = timed(c, "k_near_pick", 2.0 * b_mat + 16.0 * (double)n_q, 0, [&] { nemo::launch_near_pick(a, s); })))
    return give_up(rc);
  if (outer) {
    hipEvent_t tb = get_event(c);
    hipEventRecord(tb, s);
    c->pending.push_back({"k_near", ta, tb, b_bits + b_isect + b_mat, ops});
    ta = nullptr;
  }
  nemo::launch_to_host(c->h_near.p, cs.d_nrout.p, 16 * (uint64_t)n_q, s);  // the rows to pinned memory
  HIPCHK(c, hipEventRecord(c->ev_near, s));
  HIPCHK(c, hipEventSynchronize(c->ev_near));
  cs.near_nq = (uint32_t)n_q;
  cs.near_nc = (uint32_t)n_c;
  cs.near_done = true;
  return NEMO_OK;
}

int nemo_fetch_nearest(nemo_ctx *c, nemo_nearest *out, uint64_t cap, uint64_t *n_out) {
  if (!c) return NEMO_ERR_INVALID;
  if (c->node || !c->cs.near_done)
    return fail(c, NEMO_ERR_STATE, "nemo_fetch_nearest before nemo_nearest_runs (or after a later nemo_load_corpus)");
  const uint64_t n = c->cs.near_nq;  // no ensure_whole: reads the last call's host rows, no graph
  if (n_out) *n_out = n;
  if (!out) return NEMO_OK;
  if (cap < n) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  if (n) memcpy(out, c->h_near.p, n * sizeof(nemo_nearest));
  return NEMO_OK;
}

int nemo_fetch_label_distances(nemo_ctx *c, uint32_t q_lo, uint32_t q_hi, uint32_t *out, uint64_t cap) {
  if (!c) return NEMO_ERR_INVALID;
  if (c->node || !c->cs.near_done)
    return fail(c, NEMO_ERR_STATE, "nemo_fetch_label_distances before nemo_nearest_runs (or after a later nemo_load_corpus)");
  if (q_lo > q_hi || q_hi > c->cs.near_nq)
    return fail(c, NEMO_ERR_INVALID, "query rows [%u, %u) out of range (%u queries)", q_lo, q_hi, c->cs.near_nq);
  const uint64_t n = (uint64_t)(q_hi - q_lo) * c->cs.near_nc;
  if (!n) return NEMO_OK;
  if (!out) return NEMO_ERR_INVALID;
  if (cap < n) return fail(c, NEMO_ERR_INVALID, "capacity too small");
  HIPCHK(c, hipSetDevice(c->device));
  if (int rw = ensure_whole(c)) return rw;  // may read any graph
  HIPCHK(c, hipMemcpyAsync(out, c->cs.d_nrmat.p + (size_t)q_lo * c->cs.near_nc, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return NEMO_OK;
}

}  // extern "C"
