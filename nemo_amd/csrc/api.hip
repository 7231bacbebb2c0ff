// api.hip — the C ABI of libnemohip (include/nemohip.h): context, device
// memory layout of a loaded corpus, phase orchestration, result fetches and
// per-kernel HIP-event timing.  No CPU fallback exists: every analysis result
// comes from the gfx950 kernels in k_*.hip.
#include "ctx.h"
#include "load_host.h"

static void set_lds_tier(nemo_ctx *c);
static void set_global_block(nemo_ctx *c);
static void set_build_tier(nemo_ctx *c);

// the kernels' graph list: the representatives while the option is on and the load found duplicates
static void set_graph_dedup(nemo_ctx *c) {
  const bool on = c->opt.graph_dedup && c->cs.gd_npairs != 0;
  c->cs.dc.dd_list = on ? c->cs.d_gd_list : nullptr;
  c->cs.dc.dd_n = on ? c->cs.gd_nlist : 0;
  c->cs.dc.dd_rep = on ? c->cs.d_gd_rep : nullptr;
  // ... and the runs' list: the representative runs, under the same conditions and option proto_dedup
  const bool runs = on && c->opt.proto_dedup && c->cs.gd_nrpairs != 0;
  c->cs.dc.run_list = runs ? c->cs.d_gd_rlist : nullptr;
  c->cs.dc.run_pairs = runs ? c->cs.d_gd_rpairs : nullptr;
  c->cs.dc.run_n = runs ? c->cs.gd_nrlist : 0;
  c->cs.dc.run_npairs = runs ? c->cs.gd_nrpairs : 0;
}
// a replicate pass behind `phase`'s kernel (k_gdedup.hip); nothing without duplicates
static int replicate(nemo_ctx *c, int phase) {
  if (!c->cs.dc.dd_list) return NEMO_OK;
  return timed(c, "k_replicate", c->cs.gd_bytes[phase], 0,
               [&] { nemo::launch_replicate(c->cs.dc, c->cs.d_gd_pairs, c->cs.gd_npairs, phase, c->stream); });
}

static void tiers_reset(nemo_ctx *c) {
  c->cs.tiers_ok = c->cs.tiers_pending = false;
  c->cs.tiers_run = 0;
}
// tier k's worklist is known to be empty (no launch needed)
static bool tier_empty(nemo_ctx *c, int k) {
  if (!c->cs.tiers_ok && c->cs.tiers_pending && hipEventQuery(c->ev_tiers) == hipSuccess) {
    for (int i = 0; i < 3; i++) c->cs.tiers[i] = c->h_tiers.p[i];
    c->cs.tiers_ok = true;
    c->cs.tiers_pending = false;
  }
  return c->cs.tiers_ok && c->cs.tiers[k] == 0;
}
// after a pass that launched all three tiers: their list counts to pinned host memory
static int tiers_capture(nemo_ctx *c, hipStream_t s) {
  if (c->cs.tiers_ok || c->cs.tiers_pending || c->cs.tiers_run != 7u || !c->cs.G) return NEMO_OK;
  int rc;
  if ((rc = c->h_tiers.grow(c, 4))) return rc;
  if ((rc = ensure_event(c, &c->ev_tiers))) return rc;
  const size_t L = (size_t)c->cs.G + 1;
  nemo::HostCopies hc;
  hc.add(c->h_tiers.p + 0, c->cs.dc.sel + 2 * L, 4);
  hc.add(c->h_tiers.p + 1, c->cs.dc.sel + L, 4);
  hc.add(c->h_tiers.p + 2, c->cs.dc.sel + 3 * L, 4);
  nemo::launch_to_host_multi(hc, s);
  HIPCHK(c, hipEventRecord(c->ev_tiers, s));
  c->cs.tiers_pending = true;
  return NEMO_OK;
}

// ---- the node context's facade (node.h) ----
nemo_ctx *ctx_new_facade(Node *n) {
  nemo_ctx *c = new nemo_ctx();
  c->node = n;
  return c;
}
void ctx_delete_facade(nemo_ctx *c) { delete c; }

extern "C" {

int nemo_abi_version(void) { return NEMOHIP_ABI_VERSION; }

int nemo_host_register(const void *ptr, uint64_t bytes) {
  if (!ptr || !bytes) return NEMO_ERR_INVALID;
  return hipHostRegister(const_cast<void *>(ptr), (size_t)bytes, hipHostRegisterDefault) == hipSuccess ? NEMO_OK
                                                                                                       : NEMO_ERR_HIP;
}
int nemo_host_unregister(const void *ptr) {
  if (!ptr) return NEMO_ERR_INVALID;
  return hipHostUnregister(const_cast<void *>(ptr)) == hipSuccess ? NEMO_OK : NEMO_ERR_HIP;
}

// Run sharding: longest-processing-time-first over the runs'
// node + edge counts (both graphs), ties by run index; each run goes to the
// least-loaded part so far (ties by part index).  Deterministic, so every
// rank of a torchrun job and the in-library node context agree.
int nemo_partition_runs(const nemo_corpus *in, uint32_t n_parts, uint32_t *part_of_run) {
  if (!in || !part_of_run || n_parts == 0 || (in->n_runs && (!in->node_off || !in->edge_off))) return NEMO_ERR_INVALID;
  const uint32_t R = in->n_runs;
  std::vector<std::pair<uint64_t, uint32_t>> w(R);
  for (uint32_t r = 0; r < R; r++)
    w[r] = {in->node_off[2 * r + 2] - in->node_off[2 * r] + in->edge_off[2 * r + 2] - in->edge_off[2 * r], r};
  std::sort(w.begin(), w.end(), [](const std::pair<uint64_t, uint32_t> &a, const std::pair<uint64_t, uint32_t> &b) {
    return a.first != b.first ? a.first > b.first : a.second < b.second;
  });
  using Load = std::pair<uint64_t, uint32_t>;  // (load, part): min-heap
  std::vector<Load> heap(n_parts);
  for (uint32_t p = 0; p < n_parts; p++) heap[p] = {0, p};
  auto cmp = [](const Load &a, const Load &b) { return a > b; };
  std::make_heap(heap.begin(), heap.end(), cmp);
  for (auto &x : w) {
    std::pop_heap(heap.begin(), heap.end(), cmp);
    part_of_run[x.second] = heap.back().second;
    heap.back().first += x.first;
    std::push_heap(heap.begin(), heap.end(), cmp);
  }
  return NEMO_OK;
}

int nemo_ctx_create(int device, nemo_ctx **out) {
  if (!out) return NEMO_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return NEMO_ERR_NOGPU;
  if (device < 0 || device >= n) return NEMO_ERR_INVALID;
  nemo_ctx *c = new nemo_ctx();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return NEMO_ERR_HIP;
  }
  c->stream = c->own;
  *out = c;
  return NEMO_OK;
}

static void release_corpus(nemo_ctx *c) {
  if (getenv("NEMO_LOAD_DEBUG"))
    fprintf(stderr, "release_corpus: since load %llu dalloc, %llu dfree, size hash %016llx\n",
            (unsigned long long)c->call_dalloc_n, (unsigned long long)c->call_dfree_n, (unsigned long long)c->call_hash);
  drop_cache(c);  // blocks no allocation took since the last load
  for (void *p : c->allocs) {  // kept for the next load
    auto b = c->alloc_bytes.find(p);
    if (b != c->alloc_bytes.end()) c->cache.emplace(b->second, p);
    else hipFree(p);
  }
  c->allocs.clear();
  c->cs = CorpusState{};  // every pointer into those blocks, and what was computed from them
}

void nemo_ctx_destroy(nemo_ctx *c) {
  if (!c) return;
  if (c->node) {
    node_destroy(c->node);
    ctx_delete_facade(c);
    return;
  }
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  if (c->copy) hipStreamSynchronize(c->copy);
  if (c->aux) hipStreamSynchronize(c->aux);
  release_corpus(c);
  drop_cache(c);
  std::vector<hipEvent_t> ev(c->ev_pool);
  for (auto &p : c->pending) ev.insert(ev.end(), {p.a, p.b});
  ev.insert(ev.end(), c->ev_up.begin(), c->ev_up.end());
  for (hipEvent_t *e : c->events) ev.push_back(*e);
  ev.insert(ev.end(), c->ev_state, c->ev_state + NEMO_STAGE_SLICES_MAX);
  ev.insert(ev.end(), c->ev_ready, c->ev_ready + NEMO_STAGE_SLICES_MAX);
  for (hipEvent_t e : ev)
    if (e) hipEventDestroy(e);
  for (void **h : c->pinned)
    if (*h) hipHostFree(*h);
  for (hipStream_t *s : c->streams)  // `own` last
    if (*s) {
      hipStreamSynchronize(*s);
      hipStreamDestroy(*s);
    }
  delete c;
}

const char *nemo_last_error(const nemo_ctx *c) { return c ? c->err.c_str() : "null context"; }

int nemo_set_stream(nemo_ctx *c, void *stream) {
  DISPATCH(node_set_stream(c, stream));
  if (!c) return NEMO_ERR_INVALID;
  c->stream = stream ? (hipStream_t)stream : c->own;
  return NEMO_OK;
}

int nemo_set_option(nemo_ctx *c, const char *name, int64_t value) {
  DISPATCH(node_set_option(c, name, value));
  if (!c || !name) return NEMO_ERR_INVALID;
  if (c->cs.gd_stale) {  // the kernels after an option change may read any graph's slices
    HIPCHK(c, hipSetDevice(c->device));
    if (int rw = ensure_whole(c)) return rw;
  }
  tiers_reset(c);  // any option may move graphs between tiers
  c->cs.ms_fused = false;  // ... and the fused tail's graphs were chosen under the old caps
  // the hand-over orders itself behind everything queued so far again, not behind nemo_simplify's events
  c->cs.flags_final = c->cs.chains_final = false;
  if (!strcmp(name, "chains_lds_max")) {
    c->opt.hcap_limit = value < 0 ? 0xFFFFFFFFu : (uint32_t)value;
    c->cs.dc.hcap_limit = c->opt.hcap_limit;
    return NEMO_OK;
  }
  if (!strcmp(name, "build_lds_max")) {
    c->opt.build_limit = value < 0 ? 0xFFFFFFFFu : (uint32_t)value;
    if (c->cs.loaded) set_build_tier(c);
    return NEMO_OK;
  }
  if (!strcmp(name, "graph_lds_max")) {
    if (c->cs.loaded) {
      HIPCHK(c, hipSetDevice(c->device));
      if (int rm = ensure_marked(c)) return rm;  // the deferred set depends on the tier caps
    }
    c->opt.lds_limit = value < 0 ? 0xFFFFFFFFu : (uint32_t)value;
    if (c->cs.loaded) set_lds_tier(c);
    return NEMO_OK;
  }
  if (!strcmp(name, "diff_legacy")) {  // 1: CreateNaiveDiffProv by the one-workgroup-per-entry kernels
    c->opt.diff_legacy = value > 0;
    return NEMO_OK;
  }
  if (!strcmp(name, "diff_window")) {  // test knob of the multi-entry diff's walks: 0, 1 or 2
    if (value < 0 || value > 2) return fail(c, NEMO_ERR_INVALID, "diff_window: 0, 1 or 2");
    c->opt.diff_window = (uint32_t)value;
    return NEMO_OK;
  }
  if (!strcmp(name, "stage_sdma")) {
    c->opt.stage_sdma = value > 0;
    return NEMO_OK;
  }
  if (!strcmp(name, "stage_aux")) {  // 0: the hand-over kernels on the context's stream
    c->opt.stage_on_aux = value != 0;
    return NEMO_OK;
  }
  if (!strcmp(name, "diff_aux")) {  // 0: the diff kernels on the context's stream, in call order
    c->opt.diff_on_aux = value != 0;
    return NEMO_OK;
  }
  if (!strcmp(name, "pull_aux")) {  // 0: pulls on the context's stream, after everything queued before them
    c->opt.pull_on_aux = value != 0;
    return NEMO_OK;
  }
  if (!strcmp(name, "stage_cus")) {  // takes effect when the copy stream is created (first stage)
    c->opt.stage_cus = value < 0 ? 8u : (uint32_t)value;
    return NEMO_OK;
  }
  if (!strcmp(name, "stage_blocks")) {
    c->opt.stage_blocks = value < 0 ? 0u : (uint32_t)value;
    return NEMO_OK;
  }
  if (!strcmp(name, "stage_slices")) {  // 1..8 slices of the node state, each with its own copy
    c->opt.stage_slices = stage::clamp_slices(value, NEMO_STAGE_SLICES_DEFAULT);
    return NEMO_OK;
  }
  if (!strcmp(name, "stage_pair_slices")) {  // ... and of the chain pairs
    c->opt.stage_pair_slices = stage::clamp_slices(value, NEMO_STAGE_PAIR_SLICES_DEFAULT);
    return NEMO_OK;
  }
  if (!strcmp(name, "stage_slice_ratio")) {  // 1: equal state slices; r: each r times the one before
    c->opt.stage_ratio = value < 0 ? NEMO_STAGE_RATIO_DEFAULT : (uint32_t)std::min<int64_t>(std::max<int64_t>(value, 1), NEMO_STAGE_RATIO_MAX);
    return NEMO_OK;
  }
  if (!strcmp(name, "chains_glob_block")) {  // 0 (by corpus), 256 or 512; takes effect at the next load
    if (value != 0 && value != 256 && value != 512) return fail(c, NEMO_ERR_INVALID, "chains_glob_block: 0, 256 or 512");
    c->opt.glob_block_force = (uint32_t)value;
    return NEMO_OK;
  }
  if (!strcmp(name, "chains_glob_stop")) {  // diagnostic (stamps build only; set after the load): k_chains_glob returns after phase k
    c->cs.dc.glob_stop = value < 0 ? 0u : (uint32_t)value;
    return NEMO_OK;
  }
  if (!strcmp(name, "diff_fuse")) {  // test knob: 0 runs k_dx_lp / k_dx_emit after whole-graph walks too
    c->opt.diff_unfused = value == 0;
    return NEMO_OK;
  }
  if (!strcmp(name, "build_relax")) {  // 1: k_build's Kahn levels by relaxation sweeps first; 0 / -1: peeling
    c->opt.relax_off = value <= 0;
    c->cs.dc.bld_relax = c->opt.relax_off ? 0u : 1u;
    return NEMO_OK;
  }
  if (!strcmp(name, "build_marksimp")) {  // 1: k_build's tail; 0 / -1: k_marksimp takes every tier graph
    c->opt.ms_fuse_off = value <= 0;
    return NEMO_OK;
  }
  if (!strcmp(name, "load_async")) {  // 1: nemo_load_corpus does not wait for its kernels (checks deferred)
    c->opt.load_async = value > 0;
    return NEMO_OK;
  }
  if (!strcmp(name, "load_parts")) {  // big-graph corpora: uploads in this many parts (1: one upload, then the build)
    c->opt.load_parts = value < 1 ? 4u : (uint32_t)std::min<int64_t>(value, 64);
    return NEMO_OK;
  }
  if (!strcmp(name, "topo_ell")) {  // 1: k_topo_ell for the deep graphs (child records); 0 / -1: k_topo_deep
    c->opt.topo_ell_off = value <= 0;
    c->cs.dc.topo_ell = c->opt.topo_ell_off ? 0u : 1u;
    return NEMO_OK;
  }
  if (!strcmp(name, "chains_glob_prep")) {  // 0: no k_glob_prep (the per-graph front phases); takes effect at the next load
    c->opt.glob_prep_off = value == 0;
    return NEMO_OK;
  }
  if (!strcmp(name, "chains_glob_min_v")) {  // takes effect at the next nemo_load_corpus
    c->opt.glob_min_v = value < 0 ? ~0ull : (uint64_t)value;
    return NEMO_OK;
  }
  if (!strcmp(name, "global_block")) {  // 256, 1024, or -1 = by corpus shape (set_global_block)
    if (value != 256 && value != 1024 && value != -1) return fail(c, NEMO_ERR_INVALID, "global_block must be 256, 1024 or -1");
    c->opt.gblock_force = value < 0 ? 0u : (uint32_t)value;
    if (c->cs.loaded) set_global_block(c);
    return NEMO_OK;
  }
  if (!strcmp(name, "class_hash_bits")) {  // test knob: 0..128 low hash bits bucket the D masks (nemo_diff_classes)
    if (value < -1 || value > 128) return fail(c, NEMO_ERR_INVALID, "class_hash_bits: 0..128, or -1");
    c->opt.class_hash_bits = value < 0 ? 128 : (int)value;
    return NEMO_OK;
  }
  if (!strcmp(name, "graph_dedup")) {  // 0: every graph runs its own workgroup, nothing is replicated
    c->opt.graph_dedup = value != 0;
    set_graph_dedup(c);
    return NEMO_OK;
  }
  if (!strcmp(name, "proto_dedup")) {  // 0: k_proto_lds runs every run; 1 / -1: one run per run class
    c->opt.proto_dedup = value != 0;
    set_graph_dedup(c);
    return NEMO_OK;
  }
  if (!strcmp(name, "replicate_lazy")) {  // 0: k_build's slices reach the duplicates right behind k_build; 1 / -1: on demand
    c->opt.replicate_lazy = value != 0;
    return NEMO_OK;
  }
  if (!strcmp(name, "pull_dedup")) {  // 0: raw / simplified pulls compact every graph; 1 / -1: one graph per class
    c->opt.pull_dedup = value != 0;  // (read by the next nemo_pull_edges; a pull already queued keeps its slots)
    return NEMO_OK;
  }
  if (!strcmp(name, "dedup_hash_bits")) {  // test knob: 0..128 low hash bits bucket the graphs; takes effect at the next load
    if (value < -1 || value > 128) return fail(c, NEMO_ERR_INVALID, "dedup_hash_bits: 0..128, or -1");
    c->opt.dedup_hash_bits = value < 0 ? 128 : (int)value;
    return NEMO_OK;
  }
  if (!strcmp(name, "pair_hash_lds_max")) {  // largest label table (slots) k_lab_hash builds in LDS; 0: every table in place
    c->opt.pair_hash_lds_max = value < 0 ? LAB_HASH_LDS_SLOTS : (uint32_t)std::min<int64_t>(value, LAB_HASH_LDS_SLOTS);
    return NEMO_OK;
  }
  if (!strcmp(name, "near_bits_lds_max")) {  // largest bit row (bytes) k_near_bits builds in LDS; 0: every row in place
    c->opt.near_bits_lds_max = value < 0 ? NEAR_LDS_MAX : (uint32_t)std::min<int64_t>(value, NEAR_LDS_MAX);
    return NEMO_OK;
  }
  if (!strcmp(name, "near_ksplit")) {  // K ranges of k_near_isect; 0 / -1: by the tile count and the device
    c->opt.near_ksplit = value < 0 ? 0u : (uint32_t)std::min<int64_t>(value, NEAR_MAX_KSPLIT);
    return NEMO_OK;
  }
  if (!strcmp(name, "knock_lds_max")) {  // largest LDS image (bytes) k_ko_lds takes; 0: every graph to k_ko_glob
    c->opt.knock_lds_max = value < 0 ? KO_LDS_MAX : (uint32_t)std::min<int64_t>(value, KO_LDS_MAX);
    return NEMO_OK;
  }
  if (!strcmp(name, "cut_grid")) {  // most workgroups of the cut-set sweeps; 0 / -1: as many as are resident
    c->opt.cut_grid = value < 0 ? 0u : (uint32_t)std::min<int64_t>(value, 0x7FFFFFFF);
    return NEMO_OK;
  }
  if (!strcmp(name, "kl_grid")) {  // most workgroups of the label knock-out's sweeps; 0 / -1: as many as are resident
    c->opt.kl_grid = value < 0 ? 0u : (uint32_t)std::min<int64_t>(value, 0x7FFFFFFF);
    return NEMO_OK;
  }
  if (!strcmp(name, "kl_hitlist")) {  // 0: k_kl_lds without the hit list (V probes per chunk); 1 / -1: with it
    c->opt.kl_hitlist = value != 0;
    return NEMO_OK;
  }
  if (!strcmp(name, "wit_lds_max")) {  // largest LDS image (bytes) k_wit_lds takes; 0: every graph to k_wit_glob
    c->opt.wit_lds_max = wit::lds_max_option(value);
    return NEMO_OK;
  }
  if (!strcmp(name, "lineage_children_max")) {  // most children a level of nemo_lineage_cuts may emit; -1: the default
    const uint64_t v = lin::children_option(value);
    if (!v) return fail(c, NEMO_ERR_INVALID, "lineage_children_max must be >= %llu (-1: the default, %llu)", LIN_CHILDREN_MIN, LIN_CHILDREN_DEFAULT);
    c->opt.lin_children_max = v;
    return NEMO_OK;
  }
  if (!strcmp(name, "chains_comp_max")) {
    c->opt.comp_limit = value < 0 ? 0xFFFFFFFFu : (uint32_t)value;
    c->cs.dc.comp_limit = c->opt.comp_limit;
    return NEMO_OK;
  }
  return fail(c, NEMO_ERR_INVALID, "unknown option %s", name);
}

int nemo_set_timing(nemo_ctx *c, int enable) {
  DISPATCH(node_set_timing(c, enable));
  if (!c) return NEMO_ERR_INVALID;
  c->timing = enable != 0;
  return NEMO_OK;
}

int nemo_set_timing_groups(nemo_ctx *c, const char *groups) {
  DISPATCH(node_set_timing_groups(c, groups));
  if (!c) return NEMO_ERR_INVALID;
  c->tgroups.clear();
  for (const char *p = groups; p && *p;) {
    const char *q = strchr(p, ',');
    const size_t n = q ? (size_t)(q - p) : strlen(p);
    if (n) c->tgroups.emplace_back(p, n);
    p = q ? q + 1 : p + n;
  }
  return NEMO_OK;
}

uint64_t nemo_num_nodes(const nemo_ctx *c) { return c ? (c->node ? node_num_nodes(c) : c->cs.V) : 0; }
uint64_t nemo_num_edges(const nemo_ctx *c) { return c ? (c->node ? node_num_edges(c) : c->cs.E) : 0; }

// Workgroup size of the global-tier kernels: deep corpora (at least one graph
// in eight over 64k nodes) have few graphs per CU and long per-node passes,
// so they get 1024 threads (16 waves of memory-level parallelism per graph);
// corpora of small graphs keep 256 so the early-exit workgroups of the LDS
// tier's graphs stay cheap.
static void set_global_block(nemo_ctx *c) {
  uint32_t deep = 0;
  for (uint32_t g = 0; g < c->cs.G; g++) deep += c->cs.nv(g) >= 65536u;
  c->cs.dc.gblock = c->opt.gblock_force ? c->opt.gblock_force : ((uint64_t)deep * 8u >= c->cs.G && deep ? 1024u : NEMO_BLOCK);
}

// LDS tiers (device.h Tier): for each tiered kernel, the largest graphs,
// smallest first, whose image in that kernel's LDS layout fits LDS_TIER_BUDGET,
// i.e. two workgroups per CU.  Graphs outside a kernel's caps run its
// global-memory variant.  `graph_lds_max` caps V of every tier (test knob).
#define LDS_TIER_BUDGET (78u * 1024u)
#define NO_LEVEL_CAP 0xFFFFFFFFu
typedef uint32_t (*TierBytes)(uint32_t v, uint32_t e, uint32_t l, uint32_t words);
static Tier fit_tier(nemo_ctx *c, uint64_t vmax, uint64_t emax, uint32_t lcap, TierBytes bytes,
                     uint32_t budget = LDS_TIER_BUDGET) {
  std::vector<std::pair<uint32_t, uint32_t>> ve;
  ve.reserve(c->cs.G);
  for (uint32_t g = 0; g < c->cs.G; g++) {
    const uint64_t v = c->cs.nv(g), e = c->cs.ne(g);
    if (v <= vmax && e <= emax) ve.push_back({(uint32_t)v, (uint32_t)e});
  }
  std::sort(ve.begin(), ve.end());
  uint32_t cv = 0, ce = 0, em = 0;
  for (auto &x : ve) {
    em = std::max(em, x.second);
    const uint32_t l = std::min(x.first, lcap);
    if (bytes(x.first, em, l, c->cs.W) > budget) break;
    cv = x.first;
    ce = em;
  }
  Tier t{0, 0, 0, 0};
  if (!cv) return t;
  t.v = cv;
  t.e = ce;
  t.l = std::min(cv, lcap);
  t.bytes = bytes(cv, ce, t.l, c->cs.W);
  return t;
}

static void set_lds_tier(nemo_ctx *c) {
  // k_proto_lds: edges in source Kahn order + level offsets (<= 512 levels), node bytes, chains; three
  // 512-thread workgroups per CU
  const uint64_t vcap = std::min<uint64_t>(16384, c->opt.lds_limit), vcap_pull = std::min<uint64_t>(24u * 256u, c->opt.lds_limit);
  const Tier tp = fit_tier(
      c, vcap, 65535, 512u,
      [](uint32_t v, uint32_t e, uint32_t l, uint32_t w) { return lds_tier_bytes(v, e, l, w); },
      160u * 1024u / 3u - 256u);
  c->cs.dc.lds_v = tp.v;
  c->cs.dc.lds_e = tp.e;
  c->cs.dc.lds_l = tp.l;
  c->cs.dc.lds_bytes = tp.bytes;
  // k_marksimp: node word + two node bytes (the edge list stays in registers / HBM); (src << 16 | dst) pairs
  c->cs.dc.t_ms = fit_tier(c, vcap, 65535, NO_LEVEL_CAP, [](uint32_t v, uint32_t, uint32_t, uint32_t w) {
    return marksimp_bytes(v, w);
  });
  // k_diff_lds: u16 CSR both ways + rule bitmap + node bits (Kahn order and depths stay in HBM)
  c->cs.dc.t_diff = fit_tier(c, vcap, 65535, NO_LEVEL_CAP, [](uint32_t v, uint32_t e, uint32_t l, uint32_t) {
    return diff_lds_bytes(v, e, l);
  });
  // k_pull_lds: forward u16 CSR + liveness bitmap (per-node counts in registers: 24 nodes per thread)
  c->cs.dc.t_pull = fit_tier(c, vcap_pull, 65535, NO_LEVEL_CAP, [](uint32_t v, uint32_t e, uint32_t, uint32_t) {
    return pull_lds_bytes(v, e);
  });
  c->cs.tierV = c->cs.tierE = 0;  // k_marksimp's graphs (the deferred markConditionHolds)
  c->cs.ms_rest = c->cs.pull_rest = 0;  // graphs the per-graph global-tier kernels must take (none: not launched)
  for (uint32_t g = 0; g < c->cs.G; g++) {
    const uint64_t v = c->cs.nv(g), e = c->cs.ne(g);
    const bool ms = tier_fits(c->cs.dc.t_ms, (uint32_t)std::min<uint64_t>(v, ~0u), (uint32_t)std::min<uint64_t>(e, ~0u), 0);
    if (ms) {
      c->cs.tierV += (double)v;
      c->cs.tierE += (double)e;
    } else if (v < NEMO_CSR_BIG) {
      c->cs.ms_rest++;
    }
    if (!tier_fits(c->cs.dc.t_pull, (uint32_t)std::min<uint64_t>(v, ~0u), (uint32_t)std::min<uint64_t>(e, ~0u), 0))
      c->cs.pull_rest++;
  }
}

// k_build's LDS caps: the largest graphs, smallest first, whose build image
// (k_load.hip build_tier_bytes) keeps four workgroups on a CU.
#define BUILD_TIER_BUDGET (160u * 1024u / 4u - 64u)
static void set_build_tier(nemo_ctx *c) {
  const Tier t = fit_tier(
      c, std::min<uint64_t>(16384, c->opt.build_limit), 32u * NEMO_BLOCK, NO_LEVEL_CAP,
      [](uint32_t v, uint32_t e, uint32_t, uint32_t) { return nemo::build_tier_bytes(v, e); }, BUILD_TIER_BUDGET);
  c->cs.dc.bld_v = t.v;
  c->cs.dc.bld_e = t.e;
  c->cs.dc.bld_bytes = t.bytes;
}

// Upload parts of a corpus whose edges are mostly big graphs (nemo_load_corpus, option load_parts):
// part k = the big-list entries [b0, b1) and the edge range [e0, e1) of the graphs from big[b0] up
// to the next part's first big graph (every edge in exactly one part).
struct LoadPart {
  uint32_t b0, b1;
  uint64_t e0, e1;
};
struct LoadParts {
  std::vector<LoadPart> part;
  const uint32_t *src = nullptr, *dst = nullptr;  // the caller's edge arrays (host)
  uint32_t *es = nullptr, *ed = nullptr;          // their device copies
};

// With parts, part k's edges are copied on the upload stream and its big graphs' CSR build
// (k_csrb) is queued behind that copy alone; the host issues part k + 1's copy after queueing part
// k's kernels.  A copy from page-locked memory holds the issuing thread until it is done (~200 ms
// for a C5 batch's edges, measured), so issuing every copy first left no kernel to overlap them
// with.  The rest of the load (k_build, k_csr, the Kahn levels) runs behind the last part: the
// deep graphs' k_topo_deep is per-graph latency (~74 ms for any number of graphs), so one launch
// per part took 4 x 70 ms.
static int device_load(nemo_ctx *c, const LoadParts *lp = nullptr) {
  int rc;
  const bool split = c->cs.dc.n_big && lp && lp->part.size() > 1;
  nemo::launch_zero(c->cs.dc.err, c->cs.G * sizeof(uint32_t), c->stream);
  if (split) {
    for (size_t k = 0; k < lp->part.size(); k++) {
      const LoadPart &q = lp->part[k];
      if (q.e1 > q.e0) {
        HIPCHK(c, hipMemcpyAsync(lp->es + q.e0, lp->src + q.e0, (q.e1 - q.e0) * 4, hipMemcpyHostToDevice, c->up));
        HIPCHK(c, hipMemcpyAsync(lp->ed + q.e0, lp->dst + q.e0, (q.e1 - q.e0) * 4, hipMemcpyHostToDevice, c->up));
      }
      HIPCHK(c, hipEventRecord(c->ev_up[k], c->up));
      HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_up[k], 0));
      if (q.b1 == q.b0) continue;
      DevCorpus sc = c->cs.dc;
      sc.big = c->cs.dc.big + q.b0;
      sc.cb_hoff = c->cs.dc.cb_hoff + q.b0;
      sc.n_big = q.b1 - q.b0;
      const double f = (double)sc.n_big / (double)c->cs.dc.n_big;
      if ((rc = timed(c, "k_csrb", f * (16 * c->cs.bigE + 12 * c->cs.bigV), f * c->cs.bigE,
                      [&] { nemo::launch_csr_big(sc, c->cs.big_chunks, c->stream); })))
        return rc;
    }
  }
  // graphs within k_build's LDS caps vs the global tier
  double Vb = 0, Eb = 0, Vp = 0, Ep = 0;
  for (uint32_t g = 0; g < c->cs.G && c->cs.dc.bld_bytes; g++) {
    const uint64_t v = c->cs.nv(g), e = c->cs.ne(g);
    if (v <= c->cs.dc.bld_v && e <= c->cs.dc.bld_e) {
      Vb += (double)v;
      Eb += (double)e;
      if (g & 1) {
        Vp += (double)v;
        Ep += (double)e;
      }
    }
  }
  const double V = (double)c->cs.V - Vb, E = (double)c->cs.E - Eb;
  // k_build's tail runs the deferred mark + simplification (k_marksimp's work) on the edges still
  // in its registers when every k_build graph fits the tail's LDS image
  c->cs.dc.ms_fuse = !c->opt.ms_fuse_off && c->cs.dc.t_ms.bytes && c->cs.dc.bld_bytes &&
                  marksimp_bytes(c->cs.dc.bld_v, c->cs.dc.words) <= c->cs.dc.bld_bytes;
  // k_build, HBM lower bound: read the edge list (8E) and node words (4V);
  // write both column arrays (8E), both row-pointer arrays (8V), the Kahn
  // order (4V) and per-node level (4V); the level offsets are per level; post
  // graphs also their edges in source Kahn order (4E) and position offsets (4V);
  // with the tail, the node flags (1V)
  if ((rc = timed(c, "k_build", 16 * Eb + (c->cs.dc.ms_fuse ? 21 : 20) * Vb + 4 * Ep + 4 * Vp, 2 * Eb,
                  [&] { nemo::launch_build(c->cs.dc, c->stream); })))
    return rc;
  // The duplicates' scalars (redo, err, created, nlev) at once: k_load_sel reads redo and many kernels err of
  // every graph.  Their slices wait for ensure_whole when the host knows that the pass reads the slices of
  // representatives only: every graph inside k_marksimp's and the pull's LDS tiers, the three global tiers
  // known to be empty (so this is never the first pass after a load or an option), and k_proto_lds and the
  // pulls over the classes.  In any other case both go out in one launch, as before.
  c->cs.gd_stale = false;
  if (c->cs.dc.dd_list) {
    const bool lazy = c->opt.replicate_lazy && c->cs.dc.run_list && c->opt.pull_dedup && c->cs.dc.t_ms.bytes &&
                      c->cs.ms_rest == 0 && c->cs.pull_rest == 0 && tier_empty(c, 0) && tier_empty(c, 1) && tier_empty(c, 2);
    if (lazy) {
      if ((rc = timed(c, "k_build", 0, 0, [&] {
            nemo::launch_replicate(c->cs.dc, c->cs.d_gd_pairs, c->cs.gd_npairs, GD_BUILD_SCALARS, c->stream);
          })))
        return rc;
      c->cs.gd_stale = true;
    } else if ((rc = replicate(c, GD_BUILD))) {
      return rc;
    }
  }
  c->cs.ms_fused = c->cs.dc.ms_fuse != 0;
  // graphs past k_build: k_csr (one workgroup per graph) below NEMO_CSR_BIG nodes, k_csrb_* above
  const double Eg = std::max(0.0, E - c->cs.bigE), Vg = std::max(0.0, V - c->cs.bigV);
  const bool load_tier = !tier_empty(c, 0);
  if (load_tier && (rc = timed(c, "k_csr", 16 * Eg + 12 * Vg, Eg, [&] { nemo::launch_load(c->cs.dc, c->stream); })))
    return rc;
  if (load_tier) c->cs.tiers_run |= 1u;
  if (c->cs.dc.n_big && !split &&
      (rc = timed(c, "k_csrb", 16 * c->cs.bigE + 12 * c->cs.bigV, c->cs.bigE,
                  [&] { nemo::launch_csr_big(c->cs.dc, c->cs.big_chunks, c->stream); })))
    return rc;
  if ((rc = timed(c, "k_topo", 4 * E + 16 * V, E, [&] { nemo::launch_topo(c->cs.dc, c->stream, load_tier); })))
    return rc;
  // the multi-entry diff's relayout of run 0's post graph and its walk images
  // are built by the first diffprov after a load (nemo_rebuild re-derives the
  // same graph: a relayout built from an earlier Kahn order of it stays valid)
  return NEMO_OK;
}

// ---- nemo_load_corpus, in steps ----
// The order of the dalloc calls and their sizes is part of the contract: a request takes the
// smallest cached block that fits, so on a reload the order decides which array gets which block,
// and another order can make a later request miss the cache (dalloc; NEMO_LOAD_DEBUG prints both).
extern "C++" {
struct Load {  // a validated corpus on its way to the device: what the steps share
  nemo_ctx *c;
  const nemo_corpus *in;
  CorpusState &s;
  DevCorpus &d;
  const size_t V, E, G, R;
  uint64_t *no = nullptr, *eo = nullptr;  // the caller's arrays on the device
  uint32_t *word = nullptr, *label = nullptr, *rank = nullptr, *es = nullptr, *ed = nullptr;
  LoadParts lp;  // the upload plan
  int rc = NEMO_OK;
  Load(nemo_ctx *c, const nemo_corpus *in) : c(c), in(in), s(c->cs), d(s.dc), V(s.V), E(s.E), G(s.G), R(s.n_runs) {}
  template <class T>
  void A(T *&p, size_t n) {  // latches the first failure; nothing is allocated after it
    if (!rc) rc = dalloc(c, &p, n);
  }
  int load_alloc_graphs(), load_plan_glob(), load_plan_chain_tmp(), load_plan_big(), load_alloc_runs(), load_upload(),
      load_run0_tables(), load_trigger_caps();
};
}

// the CSR and scratch arrays
int Load::load_alloc_graphs() {
  A(no, G + 1);
  A(eo, G + 1);
  A(word, V + NEMO_IN_PAD);  // (k_build's clamped 16-byte loads: internal.h)
  A(label, V);
  if (s.has_rank) A(rank, V);
  A(es, E + NEMO_IN_PAD);
  A(ed, E + NEMO_IN_PAD);
  A(d.fp, V + G);
  A(d.rp, V + G);
  A(d.fc, E);
  A(d.rc, E);
  A(d.topo, V);
  A(d.lvl, V + G);
  A(d.nlv, V);
  A(d.e2, E);
  A(d.posoff, V);
  A(d.nlev, G);
  A(d.flags, V);
  A(d.sb, V);
  A(d.s_a, V + G);
  A(d.s_b, V + G);
  A(d.s_c, V + G);
  A(d.s_d, V);
  A(d.s_e, V);
  A(d.s_f, V + G);
  A(d.s_g, V + G);
  A(d.err, G);
  A(d.created, G);
  A(d.prehold, G);
  A(d.holdany, G);
  A(d.redo, G);
  return rc;
}

// deep graphs (V >= glob_min_v): k_chains_glob's per-graph scratch regions
int Load::load_plan_glob() {
  std::vector<uint64_t> off(G, ~0ull);
  uint64_t words = 0;
  for (uint32_t g = 0; g < G; g++) {
    const uint64_t v = s.nv(g), e = s.ne(g);
    if (v >= c->opt.glob_min_v && v > 0) {
      off[g] = words;
      words += (nemo::glob_words(v, e) + 63) & ~63ull;
    }
  }
  uint64_t *goff;
  if ((rc = dalloc(c, &goff, G))) return rc;
  HIPCHK(c, hipMemcpy(goff, off.data(), G * 8, hipMemcpyHostToDevice));
  d.gs_off = goff;
  // a few deep graphs: 512 threads each (their parallel phases go faster); many (more
  // than two per CU): 256, so that up to four share a CU
  uint32_t n_deep = 0;
  for (uint32_t g = 0; g < G; g++) n_deep += off[g] != ~0ull;
  d.glob_block = c->opt.glob_block_force ? c->opt.glob_block_force : (n_deep > 512 ? 256u : 512u);
  if (words && (rc = dalloc(c, &d.gscratch, words))) return rc;
  // k_glob_prep's graph list and team scratch (identity ranks only)
  std::vector<uint32_t> gl;
  for (uint32_t g = 0; g < G; g++)
    if (off[g] != ~0ull) gl.push_back(g);
  uint32_t *dgl = nullptr;
  if ((rc = dalloc(c, &dgl, gl.size()))) return rc;
  if (!gl.empty()) HIPCHK(c, hipMemcpy(dgl, gl.data(), gl.size() * 4, hipMemcpyHostToDevice));
  d.glob_list = dgl;
  d.n_glob = (uint32_t)gl.size();
  d.glob_prep = !gl.empty() && !s.has_rank && !c->opt.glob_prep_off;
  d.topo_ell = c->opt.topo_ell_off ? 0u : 1u;
  d.bld_relax = c->opt.relax_off ? 0u : 1u;
  if ((rc = dalloc(c, &d.team, nemo::glob_team_words()))) return rc;
  int ncu = 0;
  HIPCHK(c, hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device));
  d.n_cu = (uint32_t)std::max(ncu, 8);
  return NEMO_OK;
}

// the chain records, and k_chains' per-graph scratch (5 words per node) for the graphs
// k_chains_glob does not take (those keep theirs in the glob scratch)
int Load::load_plan_chain_tmp() {
  if ((rc = dalloc(c, &d.chain, 5 * V))) return rc;
  std::vector<uint64_t> off(G, 0);
  uint64_t words = 0;
  for (uint32_t g = 0; g < G; g++) {
    const uint64_t v = s.nv(g);
    off[g] = words;
    if (!(v >= c->opt.glob_min_v && v > 0)) words += 5 * v;
  }
  uint64_t *toff;
  if ((rc = dalloc(c, &toff, G))) return rc;
  HIPCHK(c, hipMemcpy(toff, off.data(), G * 8, hipMemcpyHostToDevice));
  d.tmp_off = toff;
  return dalloc(c, &d.chain_tmp, words);
}

// the worklists, and the graphs of NEMO_CSR_BIG nodes or more: the multi-workgroup CSR build's list
int Load::load_plan_big() {
  if ((rc = dalloc(c, &d.nch, G))) return rc;
  if ((rc = dalloc(c, &d.sel, 4 * (G + 1)))) return rc;
  std::vector<uint32_t> big;
  uint64_t emax = 0;
  for (uint32_t g = 0; g < G; g++) {
    const uint64_t v = s.nv(g), e = s.ne(g);
    if (v < NEMO_CSR_BIG) continue;
    big.push_back(g);
    emax = std::max(emax, e);
    s.bigV += (double)v;
    s.bigVmax = std::max<uint64_t>(s.bigVmax, v);
    s.bigE += (double)e;
  }
  uint32_t *db = nullptr;
  if ((rc = dalloc(c, &db, big.size()))) return rc;
  if (!big.empty()) HIPCHK(c, hipMemcpy(db, big.data(), big.size() * 4, hipMemcpyHostToDevice));
  d.big = db;
  d.n_big = (uint32_t)big.size();
  s.big_host = big;
  // the bucketed build's (bucket, chunk) count tables and (key, value) edge scratch
  std::vector<uint64_t> hoff(big.size() + 1, 0);
  bool fits = !big.empty();
  for (size_t b = 0; b < big.size(); b++) {
    const uint32_t g = big[b];
    const uint64_t v = s.nv(g), e = s.ne(g);
    const uint64_t nbk = (v + CB_NB - 1) / CB_NB, nck = (e + CB_CHUNK - 1) / CB_CHUNK;
    fits &= nbk <= CB_MAXB;
    hoff[b + 1] = hoff[b] + std::max<uint64_t>(nbk * nck, 1);
    d.cb_maxbk = std::max<uint32_t>(d.cb_maxbk, (uint32_t)nbk);
    d.cb_maxck = std::max<uint32_t>(d.cb_maxck, (uint32_t)std::max<uint64_t>(nck, 1));
  }
  if (fits) {
    uint64_t *dh = nullptr;
    if ((rc = dalloc(c, &dh, hoff.size()))) return rc;
    HIPCHK(c, hipMemcpy(dh, hoff.data(), hoff.size() * 8, hipMemcpyHostToDevice));
    d.cb_hoff = dh;
    if ((rc = dalloc(c, &d.cb_hist, hoff.back()))) return rc;
    // keys: e2's slots (k_build writes e2 only for the graphs it builds, the
    // bucketed build takes only the others: disjoint edge ranges)
    d.cb_key = d.e2;
    if ((rc = dalloc(c, &d.cb_val, E))) return rc;
  }
  s.big_chunks = (uint32_t)std::min<uint64_t>(128, std::max<uint64_t>(1, (emax + 16383) / 16384));
  uint64_t vpost = 0;  // k_pg_* chunks: the largest post graph
  for (uint32_t g = 1; g < G; g += 2) vpost = std::max<uint64_t>(vpost, s.nv(g));
  d.pg_chunks = (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(1, vpost / 16384));
  return NEMO_OK;
}

// the chain lists and the per-run arrays
int Load::load_alloc_runs() {
  A(d.cl_first, V);
  A(d.cl_next, V);
  A(d.proto_bits, R * s.W);
  A(d.graph_tables, R * s.W);
  A(d.gate, R);
  A(s.d_owned, R);
  A(s.d_is_success, R);
  A(s.d_red, 2 * (size_t)s.T + 4);
#ifdef NEMO_STAMPS
  A(d.stamps, 16 * G);
  if (!rc) HIPCHK(c, hipMemsetAsync(d.stamps, 0, 16 * G * 8, c->stream));
#endif
  return rc;
}

// Queues the uploads and fills in DevCorpus.  A corpus whose edges are mostly in big graphs outside
// k_build's caps (the deep configs) uploads them in parts from device_load, each part's CSR build
// and Kahn levels behind its own copy: `lp` is that plan (no parts: the edges are queued here).
int Load::load_upload() {
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemcpyAsync(no, in->node_off, (G + 1) * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(eo, in->edge_off, (G + 1) * 8, hipMemcpyHostToDevice, st));
  if (V) {
    HIPCHK(c, hipMemcpyAsync(word, in->node_word, V * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(label, in->label, V * 4, hipMemcpyHostToDevice, st));
    if (rank) HIPCHK(c, hipMemcpyAsync(rank, in->id_rank, V * 4, hipMemcpyHostToDevice, st));
  }
  d.G = s.G;
  set_build_tier(c);
  const uint32_t P = c->opt.load_parts;
  bool ok = E && d.cb_hist && P > 1 && d.n_big >= 2 * P && c->opt.topo_ell_off && s.bigE >= 0.5 * (double)E;
  for (uint32_t b = 0; b < d.n_big && ok; b++) {  // no big graph of k_build's (its redo flag comes later)
    const uint32_t g = s.big_host[b];
    const uint64_t v = s.nv(g), e = s.ne(g);
    ok = !(d.bld_bytes && v <= d.bld_v && e <= d.bld_e);
  }
  if (ok) {
    if (!c->up) HIPCHK(c, hipStreamCreateWithFlags(&c->up, hipStreamNonBlocking));
    if (c->ev_up.size() < P) c->ev_up.resize(P, nullptr);
    for (uint32_t k = 0; k < P; k++) {
      if ((rc = ensure_event(c, &c->ev_up[k]))) return rc;
      LoadPart q;
      q.b0 = (uint32_t)((uint64_t)d.n_big * k / P);
      q.b1 = (uint32_t)((uint64_t)d.n_big * (k + 1) / P);
      q.e0 = k ? s.edge_off[s.big_host[q.b0]] : 0;
      q.e1 = k + 1 < P ? s.edge_off[s.big_host[q.b1]] : E;
      lp.part.push_back(q);
    }
    lp.src = in->edge_src;
    lp.dst = in->edge_dst;
    lp.es = es;
    lp.ed = ed;
  }
  if (lp.part.empty() && E) {
    HIPCHK(c, hipMemcpyAsync(es, in->edge_src, E * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(ed, in->edge_dst, E * 4, hipMemcpyHostToDevice, st));
  }
  HIPCHK(c, hipMemcpyAsync(s.d_owned, s.owned.data(), R, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(d.nch, 0, G * 4, st));
  HIPCHK(c, hipMemsetAsync(d.prehold, 0, G * 4, st));
  d.hcap_limit = c->opt.hcap_limit;
  d.comp_limit = c->opt.comp_limit;
  set_lds_tier(c);
  set_global_block(c);
  d.n_runs = s.n_runs;
  d.n_tables = s.T;
  d.words = s.W;
  d.table_pre = s.table_pre;
  d.table_post = s.table_post;
  d.node_off = no;
  d.edge_off = eo;
  d.word = word;
  d.label = label;
  d.rank = rank;
  d.esrc = es;
  d.edst = ed;
  return NEMO_OK;
}

// run 0's post goal labels (sorted list, hash, dense table) and, when every row of its post graph
// fits one walk window, the multi-entry diff's relayout buffers
int Load::load_run0_tables() {
  if (s.run0 < 0) return NEMO_OK;
  hipStream_t st = c->stream;
  const uint32_t g0 = s.g0();
  const R0Tables t = r0_tables(s, in);
  const size_t nl = t.l.size(), hcap = t.hkey.size(), nlab = t.dense.size();
  s.n_r0lab = (uint32_t)nl;
  s.r0hmask = (uint32_t)hcap - 1;
  if ((rc = dalloc(c, &s.d_r0lab, nl))) return rc;
  if ((rc = dalloc(c, &s.d_r0idx, nl))) return rc;
  if ((rc = dalloc(c, &s.d_r0hkey, hcap))) return rc;
  if ((rc = dalloc(c, &s.d_r0hval, hcap))) return rc;
  HIPCHK(c, hipMemcpyAsync(s.d_r0hkey, t.hkey.data(), hcap * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(s.d_r0hval, t.hval.data(), hcap * 4, hipMemcpyHostToDevice, st));
  if (nlab) {
    if ((rc = dalloc(c, &s.d_r0dense, nlab))) return rc;
    HIPCHK(c, hipMemcpyAsync(s.d_r0dense, t.dense.data(), nlab * 4, hipMemcpyHostToDevice, st));
    s.nlab = (uint32_t)nlab;
  }
  if (nl) {
    HIPCHK(c, hipMemcpyAsync(s.d_r0lab, t.l.data(), nl * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(s.d_r0idx, t.ix.data(), nl * 4, hipMemcpyHostToDevice, st));
  }
  HIPCHK(c, hipStreamSynchronize(st));  // the tables go out of scope
  // the multi-entry diff's relayout of g0: every row must fit one walk window
  const uint64_t nv = s.V0(), e0 = s.edge_off[g0], ne = s.E0();
  std::vector<uint32_t> din(nv, 0), dout(nv, 0);
  uint32_t maxdeg = 0;
  for (uint64_t e = e0; e < e0 + ne; e++) {
    if (in->edge_src[e] < nv) maxdeg = std::max(maxdeg, ++dout[in->edge_src[e]]);
    if (in->edge_dst[e] < nv) maxdeg = std::max(maxdeg, ++din[in->edge_dst[e]]);
  }
  s.dx_ok = nv > 0 && nv < 0xFFFFFFFFull && maxdeg <= nemo::dx_max_row();
  s.g0_maxdeg = maxdeg;
  if (!s.dx_ok) return NEMO_OK;
  nemo::DxPrep &p = s.dxp;
  p.g0 = g0;
  p.V0 = (uint32_t)nv;
  p.E0 = (uint32_t)ne;
  p.r0idx = s.d_r0idx;
  p.n_r0lab = s.n_r0lab;
  p.err0 = nullptr;  // set at the first diffprov (the error flags are allocated with the corpus)
  p.r0lab = s.d_r0lab;
  p.r0dense = nv < (1ull << 28) ? s.d_r0dense : nullptr;  // positions << 4 must fit
  A(p.tpos, nv), A(p.pnode, nv), A(p.info, nv), A(p.lbeg, nv), A(p.lend, nv), A(p.rp, nv + 1), A(p.fp, nv + 1);
  A(p.rc, ne + 4), A(p.fc, ne + 4), A(p.r0pos, nl);
  for (nemo::DxImg &m : s.dx_img) {
    A(m.nw, 1), A(m.wb, nv + 2), A(m.stepb, nv + 2), A(m.steps, 2 * nv + ne / 256 + 4), A(m.rec, ne + 4);
    A(m.moff, nv + 1), A(m.mx, ne + 1);
  }
  nemo::DxImgScratch &ts = s.dx_its;
  A(ts.fseg, nv + 1), A(ts.segpos, nv + 2), A(ts.fstep, nv + 1);
  A(ts.tsum, nemo::dx_scan_tiles((uint32_t)std::max(nv, ne) + 1));
  return rc;
}

// trigger outputs of run 0: pre rows (a, g, r) <= sum over goals of in*out
// degree, post rows (g, r) <= edges, async rules <= nodes (corrections.go:30-34,121-125)
int Load::load_trigger_caps() {
  if (s.run0 < 0) return NEMO_OK;
  const uint32_t gp = 2 * s.run0;
  const uint64_t nv = s.nv(gp);
  std::vector<uint32_t> din(nv, 0), dout(nv, 0);
  for (uint64_t e = s.edge_off[gp]; e < s.edge_off[gp + 1]; e++) {
    if (in->edge_src[e] < nv) dout[in->edge_src[e]]++;
    if (in->edge_dst[e] < nv) din[in->edge_dst[e]]++;
  }
  for (uint64_t v = 0; v < nv; v++) s.tcap[0] += (uint64_t)din[v] * dout[v];
  s.tcap[1] = s.E0();
  s.tcap[2] = nv;
  A(s.d_tpre, 3 * s.tcap[0] + 3), A(s.d_tpost, 2 * s.tcap[1] + 2), A(s.d_tasync, s.tcap[2] + 1);
  return rc;
}

// The load's duplicate classes (DESIGN.md §3 "Duplicate graphs"): a content hash per graph on the
// device, buckets and comparison rounds on the host (gdedup_host.h), every bucket confirmed by exact
// comparisons on the device, so the classes never rest on the hash.  Behind the uploads on `stream`,
// before the first k_build.  Graphs of NEMO_CSR_BIG nodes or more and the deep graphs
// (chains_glob_min_v) stay their own representatives: their kernels are not per graph.
static int load_graph_classes(nemo_ctx *c, bool dbg) {
  CorpusState &s = c->cs;
  const uint32_t G = s.G;
  const auto t0 = std::chrono::steady_clock::now();
  uint64_t *d_hash = nullptr;
  uint8_t *d_verdict = nullptr;
  int rc;
  if ((rc = dalloc(c, &d_hash, 2 * (size_t)G)) || (rc = dalloc(c, &s.d_gd_list, G)) ||
      (rc = dalloc(c, &s.d_gd_pairs, 2 * (size_t)G)) || (rc = dalloc(c, &d_verdict, G)) ||
      (rc = dalloc(c, &s.d_gd_rlist, G / 2)) || (rc = dalloc(c, &s.d_gd_rpairs, G)) || (rc = dalloc(c, &s.d_gd_rep, G)))
    return rc;
  hipStream_t st = c->stream;
  nemo::launch_gd_hash(s.dc, d_hash, st);
  std::vector<dclass::Hash> h(G);
  HIPCHK(c, hipMemcpyAsync(h.data(), d_hash, 16 * (size_t)G, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  dclass::Refiner ref(h.data(), G, c->opt.dedup_hash_bits);
  std::vector<uint32_t> pairs;
  std::vector<uint8_t> verdict;
  while (ref.next_round(pairs)) {
    const uint32_t n = (uint32_t)(pairs.size() / 2);  // < G: every pair has its own first graph
    verdict.assign(n, 0);
    if (n) {
      HIPCHK(c, hipMemcpyAsync(s.d_gd_pairs, pairs.data(), 8 * (size_t)n, hipMemcpyHostToDevice, st));
      nemo::launch_gd_cmp(s.dc, s.d_gd_pairs, n, d_verdict, st);
      HIPCHK(c, hipMemcpyAsync(verdict.data(), d_verdict, n, hipMemcpyDeviceToHost, st));
      HIPCHK(c, hipStreamSynchronize(st));
    }
    ref.verdicts(verdict.data());
  }
  std::vector<uint8_t> eligible(G);
  for (uint32_t g = 0; g < G; g++) {
    const uint64_t v = s.nv(g);
    eligible[g] = v < NEMO_CSR_BIG && v < c->opt.glob_min_v;
  }
  gdedup::Plan p = gdedup::plan(ref.rep(), eligible, s.node_off.data());
  s.gd_nlist = (uint32_t)p.list.size();
  s.gd_npairs = (uint32_t)(p.pairs.size() / 2);
  s.gd_classes = p.classes;
  s.gd_rounds = ref.rounds();
  if (s.gd_npairs) {
    HIPCHK(c, hipMemcpyAsync(s.d_gd_list, p.list.data(), 4 * p.list.size(), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(s.d_gd_pairs, p.pairs.data(), 4 * p.pairs.size(), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(s.d_gd_rep, p.rep.data(), 4 * p.rep.size(), hipMemcpyHostToDevice, st));
    // the run classes: without a duplicate graph no run is a duplicate
    gdedup::RunPlan rp = gdedup::run_plan(p.rep);
    s.gd_nrlist = (uint32_t)rp.list.size();
    s.gd_nrpairs = (uint32_t)(rp.pairs.size() / 2);
    if (s.gd_nrpairs) {
      HIPCHK(c, hipMemcpyAsync(s.d_gd_rlist, rp.list.data(), 4 * rp.list.size(), hipMemcpyHostToDevice, st));
      HIPCHK(c, hipMemcpyAsync(s.d_gd_rpairs, rp.pairs.data(), 4 * rp.pairs.size(), hipMemcpyHostToDevice, st));
    }
    HIPCHK(c, hipStreamSynchronize(st));  // the plans go out of scope
    double dv = 0, de = 0, dvp = 0, dep = 0;
    for (uint32_t k = 0; k < s.gd_npairs; k++) {
      const uint32_t g = p.pairs[2 * k];
      const double v = (double)s.nv(g), e = (double)s.ne(g);
      dv += v, de += e;
      if (g & 1) dvp += v, dep += e;
    }
    s.gd_bytes[GD_BUILD] = 2 * (4 * (5 * dv + 2 * de) + 4 * (dvp + dep));  // read and written
    s.gd_bytes[GD_MARKSIMP] = 2 * dv;
    s.gd_bytes[GD_CHAINS] = 0;
  }
  s.gd_rep = std::move(p.rep);
  set_graph_dedup(c);
  if (dbg)
    fprintf(stderr, "nemo_load_corpus: duplicate graphs: %u graphs, %u classes + %u kept apart, %u duplicates, %.1f %% of "
            "the nodes in duplicates, %u rounds, %.1f ms\n",
            G, s.gd_classes, s.gd_nlist - s.gd_classes, s.gd_npairs, s.V ? 100.0 * (double)p.dup_nodes / (double)s.V : 0.0,
            s.gd_rounds, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  return NEMO_OK;
}

int nemo_load_corpus(nemo_ctx *c, const nemo_corpus *in) {
  DISPATCH(node_load_corpus(c, in));
  if (!c || !in) return NEMO_ERR_INVALID;
  const bool dbg = getenv("NEMO_LOAD_DEBUG") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  auto ms_since = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->copy) HIPCHK(c, hipStreamSynchronize(c->copy));
  if (c->aux) HIPCHK(c, hipStreamSynchronize(c->aux));
  if (c->up) HIPCHK(c, hipStreamSynchronize(c->up));
  release_corpus(c);  // also when the checks below fail: a failed load leaves no corpus loaded
  const double t_rel = ms_since();
  c->dalloc_n = 0;
  c->dalloc_hash = 0xCBF29CE484222325ull;
  int rc;
  if ((rc = load_validate(c, in))) return c->cs = CorpusState{}, rc;  // nor the rejected corpus's sizes
  Load L(c, in);
  if ((rc = L.load_alloc_graphs()) || (rc = L.load_plan_glob()) || (rc = L.load_plan_chain_tmp()) ||
      (rc = L.load_plan_big()) || (rc = L.load_alloc_runs()) || (rc = L.load_upload()))
    return rc;
  if (dbg)
    fprintf(stderr, "nemo_load_corpus: E %zu n_big %u G %zu cb_hist %d load_parts %u -> %zu parts; sync+release %.1f ms, +alloc %.1f ms\n",
            L.E, L.d.n_big, L.G, L.d.cb_hist != nullptr, c->opt.load_parts, L.lp.part.size(), t_rel, ms_since());
  if ((rc = L.load_run0_tables()) || (rc = L.load_trigger_caps())) return rc;
  if (dbg)
    fprintf(stderr, "nemo_load_corpus: host part done %.1f ms; %u dalloc calls, size hash %016llx\n", ms_since(),
            (unsigned)c->dalloc_n, (unsigned long long)c->dalloc_hash);
  // not with load_async (the pass waits for its hashes) nor with an upload in parts (the edges
  // arrive inside device_load; those corpora are big graphs, which are kept apart anyway)
  if (c->opt.graph_dedup && !c->opt.load_async && L.lp.part.empty() && L.G > 1 && (rc = load_graph_classes(c, dbg)))
    return rc;
  if ((rc = device_load(c, L.lp.part.empty() ? nullptr : &L.lp))) return rc;
  if (c->opt.load_async) {
    c->cs.load_check_pending = true;  // the checks wait on `stream` at the next call that reads the graphs
  } else if ((rc = check_graph_errors(c))) {
    return rc;
  }
  if (dbg) fprintf(stderr, "nemo_load_corpus: done %.1f ms\n", ms_since());
  c->cs.loaded = true;
  c->call_dalloc_n = c->call_dfree_n = 0;  // the per-call requests are counted from here (release_corpus)
  c->call_hash = 0xCBF29CE484222325ull;
  return NEMO_OK;
}

int nemo_rebuild(nemo_ctx *c) {
  DISPATCH(node_rebuild(c));
  if (!c) return NEMO_ERR_INVALID;
  if (!c->cs.loaded) return fail(c, NEMO_ERR_STATE, "no corpus loaded");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = ensure_load_checked(c);
  if (rc) return rc;
  rc = guard_staged(c);
  if (rc) return rc;
  if ((rc = join_aux(c))) return rc;  // the diff kernels read the graphs rebuilt here
  rc = device_load(c);
  if (rc) return rc;
  c->cs.marked = c->cs.simplified = c->cs.protos_done = c->cs.trig_done = false;
  c->cs.mark_pending = false;
  c->cs.dc_done = false;
  return NEMO_OK;
}

int nemo_mark_holds(nemo_ctx *c) {
  DISPATCH(node_mark_holds(c));
  if (!c) return NEMO_ERR_INVALID;
  if (!c->cs.loaded) return fail(c, NEMO_ERR_STATE, "nemo_mark_holds before nemo_load_corpus");
  HIPCHK(c, hipSetDevice(c->device));
  // no ensure_whole: k_mark / k_mw_mark_* read the build outputs of no duplicate while the slices are stale (device_load)
  if (int rl = ensure_load_checked(c)) return rl;
  const double V = (double)c->cs.V - c->cs.tierV, E = (double)c->cs.E - c->cs.tierE;
  int rc = guard_staged(c);
  if (rc) return rc;
  const bool defer = c->cs.dc.t_ms.bytes != 0;
  rc = timed(c, "k_mark", 8 * E + 13 * V, 2 * E,
             [&] { nemo::launch_mark(c->cs.dc, defer, c->stream, !defer || c->cs.ms_rest); });
  if (rc) return rc;
  c->cs.mark_pending = defer;
  c->cs.marked = true;
  c->cs.simplified = c->cs.protos_done = c->cs.trig_done = false;
  return NEMO_OK;
}

int nemo_simplify(nemo_ctx *c) {
  DISPATCH(node_simplify(c));
  if (!c) return NEMO_ERR_INVALID;
  if (!c->cs.marked) return fail(c, NEMO_ERR_STATE, "nemo_simplify before nemo_mark_holds");
  HIPCHK(c, hipSetDevice(c->device));
  // no ensure_whole: k_marksimp, k_chains and the replicates read the build outputs of representatives only (device_load)
  int rc = guard_staged(c);
  if (rc) return rc;
  if (c->cs.mark_pending) {
    const double V = c->cs.tierV, E = c->cs.tierE, Vg = (double)c->cs.V - V, Eg = (double)c->cs.E - E;
    // k_build's tail did its graphs (ms_fused); an empty load tier means it took every graph
    // (none past its caps or handed back), so nothing is left for k_marksimp
    const bool skip_built = c->cs.ms_fused;
    if (!(skip_built && tier_empty(c, 0)) &&
        (rc = timed(c, "k_marksimp", 8 * E + 5 * V, 5 * E,
                    [&] { nemo::launch_marksimp(c->cs.dc, c->stream, skip_built); })))
      return rc;
    if ((rc = replicate(c, GD_MARKSIMP))) return rc;  // also what k_build's tail wrote (ms_fused)
    rc = timed(c, "k_simplify", 8 * Eg + 14 * Vg, 2 * Eg,
               [&] { nemo::launch_simplify(c->cs.dc, true, c->stream, c->cs.ms_rest != 0); });
    if (rc) return rc;
    c->cs.mark_pending = false;
  } else {
    const double V = (double)c->cs.V, E = (double)c->cs.E;
    rc = timed(c, "k_simplify", 8 * E + 14 * V, 2 * E, [&] { nemo::launch_simplify(c->cs.dc, false, c->stream); });
    if (rc) return rc;
  }
  c->cs.ms_fused = false;  // consumed: the chain cover marks the flags, a later simplification recomputes them
  if ((rc = ensure_event(c, &c->ev_flags))) return rc;
  HIPCHK(c, hipEventRecord(c->ev_flags, c->stream));  // the flags are final (the chain cover reads them)
  c->cs.flags_final = true;
  const double V = (double)c->cs.V, E = (double)c->cs.E;
  // reads: flags 1 + Kahn level 4 + node word 4 (+ ID rank 4) per node, the edge list 8 per edge
  const bool chain_tiers = !tier_empty(c, 1);
  rc = timed(c, "k_chains", (c->cs.has_rank ? 13 : 9) * V + 8 * E, 0,
             [&] { nemo::launch_chains(c->cs.dc, c->stream, chain_tiers, c->cs.d_gd_pairs, c->cs.gd_npairs); });
  if (rc) return rc;
  if (chain_tiers) c->cs.tiers_run |= 2u;
  if ((rc = ensure_event(c, &c->ev_simp))) return rc;
  HIPCHK(c, hipEventRecord(c->ev_simp, c->stream));  // a simplified pull on `aux` starts here
  c->cs.chains_final = true;  // ... and the staged chain pairs (nemo_stage_simplified)
  c->cs.simplified = true;
  c->cs.protos_done = false;
  return NEMO_OK;
}

size_t nemo_reduce_len(const nemo_ctx *c) { return c ? (c->node ? node_reduce_len(c) : 2 * (size_t)c->cs.T + 4) : 0; }

int nemo_protos_partial(nemo_ctx *c, const uint32_t *success_iters, size_t n_success, uint32_t *d_red) {
  DISPATCH(node_protos_partial(c, success_iters, n_success, d_red));
  if (!c || (!success_iters && n_success)) return NEMO_ERR_INVALID;
  if (!c->cs.simplified) return fail(c, NEMO_ERR_STATE, "nemo_protos_partial before nemo_simplify");
  if (!d_red) d_red = c->cs.d_red;  // single-process callers use the context's own vector
  HIPCHK(c, hipSetDevice(c->device));
  // no ensure_whole: k_proto_lds reads a post graph's build outputs through its representative; k_reduce reads none
  if (c->cs.red_staged) {  // a staged copy of an older vector: wait for it, then forget it
    HIPCHK(c, hipEventSynchronize(c->ev_red));
    c->cs.red_staged = nullptr;
  }
  if (int re = ensure_event(c, &c->ev_up_succ)) return re;
  HIPCHK(c, hipEventSynchronize(c->ev_up_succ));  // the previous upload has landed (at once if there was none)
  int rg = c->h_succ.grow(c, std::max<uint64_t>(c->cs.n_runs, 1));
  if (rg) return rg;
  uint8_t *succ = c->h_succ.p;
  memset(succ, 0, c->cs.n_runs);
  uint32_t first = NEMO_NONE;
  for (size_t i = 0; i < n_success; i++) {
    auto f = c->cs.it2run.find(success_iters[i]);
    if (f == c->cs.it2run.end()) continue;  // another rank's run
    succ[f->second] = 1;
    if (i == 0) first = f->second;
  }
  hipStream_t s = c->stream;
  // k_proto first: it is what the analysis stream has ready when a bulk
  // staging copy starts beside it (a kernel queued behind the copy's start
  // waits for the copy's blit to drain); the reduction's inputs follow it
  // post graphs only (HBM lower bound): edges in source Kahn order 4E, node word 4V, flags 1V
  const double V = c->cs.postV, E = c->cs.postE;
  const bool proto_tier = !tier_empty(c, 2);
  int rc = timed(c, "k_proto", 4 * E + 5 * V, 2 * E, [&] { nemo::launch_proto(c->cs.dc, s, proto_tier); });
  if (rc) return rc;
  if (proto_tier) c->cs.tiers_run |= 4u;
  if ((rc = tiers_capture(c, s))) return rc;
  nemo::launch_to_host(c->cs.d_is_success, succ, c->cs.n_runs, s);  // pinned -> device by a copy kernel (no blit queue)
  HIPCHK(c, hipEventRecord(c->ev_up_succ, s));
  nemo::launch_zero(d_red, nemo_reduce_len(c) * 4, s);
  rc = timed(c, "k_reduce", (double)c->cs.n_runs * (c->cs.W * 8 + 8), 0,
             [&] { nemo::launch_reduce(c->cs.dc, c->cs.d_is_success, c->cs.d_owned, first, d_red, s); });
  if (rc) return rc;
  // per-run table bitsets -> pinned host (nemo_fetch_run_tables)
  const uint64_t rw = (uint64_t)c->cs.n_runs * c->cs.W;
  if ((rc = ensure_event(c, &c->ev_protos))) return rc;
  if ((rc = c->h_tab.grow(c, 2 * rw + 1))) return rc;
  nemo::HostCopies hc;
  hc.add(c->h_tab.p, c->cs.dc.proto_bits, rw * 4);
  hc.add(c->h_tab.p + rw, c->cs.dc.graph_tables, rw * 4);
  nemo::launch_to_host_multi(hc, s);
  HIPCHK(c, hipEventRecord(c->ev_protos, s));
  c->cs.protos_done = true;
  return NEMO_OK;
}

int nemo_reduce_interpret(const uint32_t *red, uint32_t T, uint32_t table_post, uint32_t *achieved, uint32_t *inter,
                          uint32_t *n_inter, uint32_t *uni, uint32_t *n_union) {
  if (!red) return NEMO_ERR_INVALID;
  uint32_t ni = 0, nu = 0;
  if (red[2 * T + 1]) {  // `longest` is only set inside the loop over list0 (prototype.go:80-103)
    for (uint32_t t = 0; t < T; t++) {
      if (t == table_post) continue;  // != condition (prototype.go:106,120)
      if (red[T + t] && red[t] == red[2 * T]) {  // foundIn == achvdCond (prototype.go:106)
        if (inter) inter[ni] = t;
        ni++;
      }
      if (red[t] > 0) {
        if (uni) uni[nu] = t;
        nu++;
      }
    }
  }
  if (achieved) *achieved = red[2 * T];
  if (n_inter) *n_inter = ni;
  if (n_union) *n_union = nu;
  return NEMO_OK;
}

static int protos_stage(nemo_ctx *c, const uint32_t *d_red) {
  int rc;
  if ((rc = ensure_event(c, &c->ev_red))) return rc;
  if (c->cs.red_staged) HIPCHK(c, hipEventSynchronize(c->ev_red));  // h_red may be in flight
  if ((rc = c->h_red.grow(c, 2 * (uint64_t)c->cs.T + 4))) return rc;
  nemo::launch_to_host(c->h_red.p, d_red, (2 * (uint64_t)c->cs.T + 4) * 4, c->stream);
  HIPCHK(c, hipEventRecord(c->ev_red, c->stream));
  c->cs.red_staged = d_red;
  return NEMO_OK;
}

int nemo_protos_stage(nemo_ctx *c, const uint32_t *d_red) {
  if (!c) return NEMO_ERR_INVALID;
  if (c->node) return NEMO_OK;  // the node context reduces inside nemo_protos_finalize
  if (!d_red) d_red = c->cs.d_red;
  if (!d_red) return fail(c, NEMO_ERR_STATE, "nemo_protos_stage before nemo_load_corpus");
  if (!c->cs.protos_done) return fail(c, NEMO_ERR_STATE, "nemo_protos_stage before nemo_protos_partial");
  HIPCHK(c, hipSetDevice(c->device));
  // no ensure_whole: reads no graph
  return protos_stage(c, d_red);
}

int nemo_protos_finalize(nemo_ctx *c, const uint32_t *d_red, uint32_t *achieved, uint32_t *inter,
                         uint32_t *n_inter, uint32_t *uni, uint32_t *n_union, uint64_t *pre_holds,
                         uint32_t *n_runs_total) {
  DISPATCH(node_protos_finalize(c, d_red, achieved, inter, n_inter, uni, n_union, pre_holds, n_runs_total));
  if (!c) return NEMO_ERR_INVALID;
  if (!d_red) d_red = c->cs.d_red;
  if (!d_red) return fail(c, NEMO_ERR_STATE, "nemo_protos_finalize before nemo_load_corpus");
  HIPCHK(c, hipSetDevice(c->device));
  // no ensure_whole: reads no graph
  const uint32_t T = c->cs.T;
  int rc;
  if (c->cs.red_staged != d_red && (rc = protos_stage(c, d_red))) return rc;
  HIPCHK(c, hipEventSynchronize(c->ev_red));
  c->cs.red_staged = nullptr;  // consumed: the next finalize copies again unless staged again
  const uint32_t *red = c->h_red.p;
  if (pre_holds) *pre_holds = red[2 * T + 2];
  if (n_runs_total) *n_runs_total = red[2 * T + 3];
  return nemo_reduce_interpret(red, T, c->cs.table_post, achieved, inter, n_inter, uni, n_union);
}

int nemo_fetch_reduce(nemo_ctx *c, uint32_t *out, uint64_t cap) {
  DISPATCH(node_fetch_reduce(c, out, cap));
  if (!c || !out) return NEMO_ERR_INVALID;
  if (!c->cs.protos_done) return fail(c, NEMO_ERR_STATE, "nemo_fetch_reduce before nemo_protos_partial");
  const uint64_t n = 2 * (uint64_t)c->cs.T + 4;
  if (cap < n) return fail(c, NEMO_ERR_INVALID, "capacity %llu < %llu", (unsigned long long)cap, (unsigned long long)n);
  HIPCHK(c, hipSetDevice(c->device));
  if (int rw = ensure_whole(c)) return rw;  // may read any graph
  HIPCHK(c, hipMemcpyAsync(out, c->cs.d_red, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return NEMO_OK;
}

int nemo_prototypes(nemo_ctx *c, const uint32_t *success_iters, size_t n_success, uint32_t *achieved,
                    uint32_t *inter, uint32_t *n_inter, uint32_t *uni, uint32_t *n_union) {
  if (!c) return NEMO_ERR_INVALID;
  if (n_success == 0)
    return fail(c, NEMO_ERR_INVALID, "no successful runs: extractProtos indexes iterProv[0] (prototype.go:80)");
  int rc = nemo_protos_partial(c, success_iters, n_success, nullptr);  // the context's own vector
  if (rc) return rc;
  return nemo_protos_finalize(c, nullptr, achieved, inter, n_inter, uni, n_union, nullptr, nullptr);
}

int nemo_fetch_run_tables(nemo_ctx *c, int which, uint32_t *out, uint64_t cap) {
  DISPATCH(node_fetch_run_tables(c, which, out, cap));
  if (!c || !out) return NEMO_ERR_INVALID;
  if (!c->cs.protos_done) return fail(c, NEMO_ERR_STATE, "run tables before nemo_protos_partial");
  const uint64_t n = (uint64_t)c->cs.n_runs * c->cs.W;
  if (cap < n) return fail(c, NEMO_ERR_INVALID, "capacity %llu < %llu", (unsigned long long)cap, (unsigned long long)n);
  HIPCHK(c, hipSetDevice(c->device));
  // no ensure_whole: reads the per-run table sets, no graph
  HIPCHK(c, hipEventSynchronize(c->ev_protos));
  memcpy(out, c->h_tab.p + (which == 0 ? 0 : n), n * 4);
  return NEMO_OK;
}

int nemo_missing_from(nemo_ctx *c, uint32_t failed_iter, const uint32_t *proto, uint32_t n_proto, uint32_t *out,
                      uint32_t *n_out) {
  DISPATCH(node_missing_from(c, failed_iter, proto, n_proto, out, n_out));
  if (!c || (!proto && n_proto)) return NEMO_ERR_INVALID;
  if (!c->cs.protos_done) return fail(c, NEMO_ERR_STATE, "nemo_missing_from before prototypes");
  uint32_t r;
  int rc = run_index(c, failed_iter, &r);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rw = ensure_whole(c)) return rw;  // may read any graph
  std::vector<uint32_t> bits(c->cs.W);
  HIPCHK(c, hipMemcpyAsync(bits.data(), c->cs.dc.graph_tables + (size_t)r * c->cs.W, c->cs.W * 4, hipMemcpyDeviceToHost,
                           c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  uint32_t n = 0;
  for (uint32_t i = 0; i < n_proto; i++) {
    const uint32_t t = proto[i];
    const bool have = t < c->cs.T && ((bits[t >> 5] >> (t & 31)) & 1u);
    if (!have) {
      if (out) out[n] = t;
      n++;
    }
  }
  if (n_out) *n_out = n;
  return NEMO_OK;
}

// Debug/inspection: copy `bytes` bytes at byte `offset` of an internal device array.
int nemo_debug_copy(nemo_ctx *c, const char *name, void *out, uint64_t offset, uint64_t bytes) {
  DISPATCH(node_debug_copy(c, name, out, offset, bytes));
  if (!c || !name || !out) return NEMO_ERR_INVALID;
  const void *base = nullptr;
  const std::string n(name);
  if (n == "topo") base = c->cs.dc.topo;
  else if (n == "lvl") base = c->cs.dc.lvl;
  else if (n == "nlv") base = c->cs.dc.nlv;
  else if (n == "diff_tpos") base = c->cs.d_dtopo.p;
  else if (n == "nlev") base = c->cs.dc.nlev;
  else if (n == "fp") base = c->cs.dc.fp;
  else if (n == "fc") base = c->cs.dc.fc;
  else if (n == "rp") base = c->cs.dc.rp;
  else if (n == "rc") base = c->cs.dc.rc;
  else if (n == "e2") base = c->cs.dc.e2;  // (entries of graphs k_build did not build: unspecified)
  else if (n == "posoff") base = c->cs.dc.posoff;
  else if (n == "flags") base = c->cs.dc.flags;
  else if (n == "dbits") base = c->cs.d_dbits.p;
  else if (n == "dmask") base = c->cs.d_dmask.p;
  else if (n == "r0lab") base = c->cs.d_r0lab;
  else if (n == "r0idx") base = c->cs.d_r0idx;
  else if (n == "stamps") base = c->cs.dc.stamps;
  else if (n == "sel") base = c->cs.dc.sel;
  else if (n == "redo") base = c->cs.dc.redo;
  else if (n == "s_a") base = c->cs.dc.s_a;
  else if (n == "gscratch") base = c->cs.dc.gscratch;
  else if (n == "gs_off") base = c->cs.dc.gs_off;
  else if (n == "run_list") base = c->cs.dc.run_list;  // the representative runs / (dup, rep) run pairs while in use
  else if (n == "run_pairs") base = c->cs.dc.run_pairs;
  else if (n == "gate") base = c->cs.dc.gate;
  else if (n == "err") base = c->cs.dc.err;  // worklists: [4][G+1] u32, count first (pulls, chains, load, protos)
  if (!base) return fail(c, NEMO_ERR_INVALID, "unknown array %s", name);
  HIPCHK(c, hipSetDevice(c->device));
  if (int rw = ensure_whole(c)) return rw;  // may read any graph
  int rc = join_aux(c);  // the diff kernels on `aux` write dbits, dmask and the Kahn relayout
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(out, (const char *)base + offset, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return NEMO_OK;
}

int nemo_synchronize(nemo_ctx *c) {
  DISPATCH(node_synchronize(c));
  if (!c) return NEMO_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->aux) HIPCHK(c, hipStreamSynchronize(c->aux));
  return NEMO_OK;
}

int nemo_timings(nemo_ctx *c, nemo_timing *out, uint32_t cap, uint32_t *n_out) {
  DISPATCH(node_timings(c, out, cap, n_out));
  if (!c) return NEMO_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = collect_timings(c)) return rc;
  uint32_t n = 0;
  for (auto &kv : c->agg) {
    if (out && n < cap) {
      memset(&out[n], 0, sizeof out[n]);
      strncpy(out[n].name, kv.first.c_str(), sizeof out[n].name - 1);
      out[n].launches = kv.second.launches;
      out[n].ms = kv.second.ms;
      out[n].bytes = kv.second.bytes;
      out[n].edges = kv.second.edges;
    }
    n++;
  }
  if (n_out) *n_out = n;
  return NEMO_OK;
}

int nemo_reset_timings(nemo_ctx *c) {
  DISPATCH(node_reset_timings(c));
  if (!c) return NEMO_ERR_INVALID;
  uint32_t n;
  int rc = nemo_timings(c, nullptr, 0, &n);
  c->agg.clear();
  return rc;
}

}  // extern "C"
