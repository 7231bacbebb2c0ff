// ctx.h — struct nemo_ctx, by lifetime (Options, CorpusState, context resources), and
// the helpers every entry point uses.  Private to the library's host side (api*.hip, node.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "cut_host.h"
#include "dclass_host.h"
#include "device.h"
#include "gdedup_host.h"
#include "internal.h"
#include "klabel_host.h"
#include "lcut_host.h"
#include "lin_host.h"
#include "lrep_host.h"
#include "knock_host.h"
#include "lgc_host.h"
#include "nearest_host.h"
#include "node.h"
#include "pairs_host.h"
#include "repair_host.h"
#include "stage_host.h"
#include "wit_host.h"

struct Agg {
  uint64_t launches = 0;
  double ms = 0, bytes = 0, edges = 0;
};
struct PendingEv {
  std::string name;
  hipEvent_t a, b;
  double bytes, edges;
};

static int fail(nemo_ctx *c, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
template <class T>
static int dalloc(nemo_ctx *c, T **p, size_t n);
static inline void dfree(nemo_ctx *c, void *p);

#define HIPCHK(c, x)                                                                               \
  do {                                                                                             \
    hipError_t e_ = (x);                                                                           \
    if (e_ != hipSuccess) return fail((c), NEMO_ERR_HIP, "%s: %s", #x, hipGetErrorString(e_));     \
  } while (0)

#define DISPATCH(call)              \
  do {                              \
    if (c && c->node) return call; \
  } while (0)

// A pinned host buffer of the context: grow-only, exactly as large as the largest request so far.
template <class T>
struct Pinned {
  T *p = nullptr;
  uint64_t cap = 0;  // elements
  int grow(nemo_ctx *c, uint64_t n) {
    if (n <= cap && p) return NEMO_OK;
    if (p) HIPCHK(c, hipHostFree(p));
    p = nullptr;
    cap = 0;
    HIPCHK(c, hipHostMalloc((void **)&p, (n ? n : 1) * sizeof(T), hipHostMallocDefault));
    cap = n;
    return NEMO_OK;
  }
  void **slot() { return (void **)&p; }  // for nemo_ctx::pinned
};

// the pull's slot tables (offset, count per slot) and region cursor: one capacity, in slots
struct PullHost {
  Pinned<uint32_t> cnt;
  Pinned<uint64_t> off;
  Pinned<unsigned long long> cur;
  uint64_t cap() const { return std::min(cnt.cap, off.cap); }
  int grow(nemo_ctx *c, uint64_t slots) {
    int rc;
    if ((rc = cnt.grow(c, slots)) || (rc = off.grow(c, slots))) return rc;
    return cur.grow(c, 1);
  }
};

// A device buffer sized per call (the diff, symmetric / pair diff, failure classes, pulls, chain gather and
// stage buffers): grow-only, the device twin of Pinned.  The block stays owned by nemo_ctx::allocs and the
// block cache, so there is no destructor and CorpusState{} is "no buffers".  A failed grow leaves {nullptr, 0}.
// Buffers that grow together are released together and then allocated in a fixed order (the dalloc / dfree
// sequence decides which cached block an array gets at the next load); the site tests the first one's capacity
// and the pointer of the one allocated last, which is set only when the whole group is.
template <class T>
struct DevBuf {
  T *p = nullptr;
  uint64_t cap = 0;  // elements
  int grow(nemo_ctx *c, uint64_t n) {
    if (p && n <= cap) return NEMO_OK;
    release(c);
    if (int rc = dalloc(c, &p, n)) return rc;
    cap = n;
    return NEMO_OK;
  }
  void release(nemo_ctx *c) {
    dfree(c, p);
    p = nullptr;
    cap = 0;
  }
};

// The buffers of a lineage search's level loop (lin_api.h's lin_levels): nemo_lineage_cuts and nemo_lineage_group_cuts
// keep one group each.  Each grows alone inside its call, to the largest request so far, behind a wait for the
// stream: kids and ktab, their contents dropped, and front, its sets kept, when a level counted more children than
// the emission buffer holds; cuts, its keys kept, and ctab, filled again from them, before a level that could overfill
// them.  ctr grows with the call's first group.
struct LinBufs {
  DevBuf<unsigned long long> ctr;  // [4] cuts so far | children counted | the next frontier's sets | unused
  DevBuf<uint64_t> kids;           // [cap][2] the children a level emits
  DevBuf<uint64_t> front;          // [cap][2] the frontier
  DevBuf<uint32_t> ktab;           // the children's table: lin::table_slots(cap)
  DevBuf<uint64_t> cuts;           // [cap][2] the cuts found so far
  DevBuf<uint32_t> ctab;           // the cuts' table: lin::table_slots(cap)
};

// The buffers and the result of a search of sets of size <= 3 over one graph (cut_api.h's node_search): nemo_min_cuts
// keeps one group, the two repair calls share another.  Each buffer grows only inside its calls, to the largest
// request so far, behind a wait for the stream: cand by the call, which fills it before the search starts; live, w[0]
// and dead together once the candidates are counted, in this order; w[1], w[2] and scan together once round 1 has
// left the live list; rows alone once the totals are known.
struct CutBufs {
  DevBuf<uint32_t> cand;           // [K] candidate position -> node
  DevBuf<uint32_t> live;           // [K] live position -> candidate position | [K] live position -> node
  DevBuf<uint64_t> w[3];           // the rounds' words, one per chunk of 64 ranks
  DevBuf<uint64_t> dead;           // the global tier: dead words of every workgroup of the launch
  DevBuf<uint32_t> scan;           // per round [chunks + 1] popcounts -> first rows; then the scan's tile sums
  DevBuf<uint32_t> rows;           // [rows][4] nemo_cut / nemo_repair
  std::vector<uint32_t> h_cand;    // the last call's candidates (nodes)
  std::vector<uint32_t> h_live;    // ... and its upload: [K1] live positions | [K1] their nodes
  uint64_t n_rows = 0;             // rows of the last call (in the call's pinned buffer)
  bool done = false;
};

// The absent set of one family of repair calls (repair_api.h's front ends): the exhaustive calls keep one, the lineage
// calls another.  Each buffer grows only inside its family's calls, to the largest request so far, behind a wait for
// the stream: d_cnt, d_tab and d_hreg before anything is counted (the pair form alone; the last two with other !=
// run 0); d_bits and the family's candidate buffer together once the graph is known (the pair form's list has room
// for every node).
struct AbsentSet {
  std::vector<uint64_t> bits;      // the last call's bitmap (the explicit form)
  nemo::LabTab tab{};              // ... and the pair form's table
  DevBuf<uint32_t> d_cnt;          // [2] the pair form's (absent sinks, Kahn levels)
  DevBuf<nemo::LabTab> d_tab;      // [1] the table k_lab_hash fills (the pair form, other != run 0)
  DevBuf<uint32_t> d_hreg;         // ... and its slots
  DevBuf<uint64_t> d_bits;         // [repair::bitmap_words(V)] the absent bitmap
};

// Graph g = nodes [node_off[g], node_off[g + 1]), edges likewise; run r's graphs are 2r (pre) and 2r + 1 (post).
struct GraphSizes {
  std::vector<uint64_t> node_off, edge_off;
  int32_t run0 = -1;
  uint64_t nv(uint32_t g) const { return node_off[g + 1] - node_off[g]; }
  uint64_t ne(uint32_t g) const { return edge_off[g + 1] - edge_off[g]; }
  uint32_t g0() const { return 2 * (uint32_t)run0 + 1; }  // run 0's post graph: only with run0 >= 0
  uint64_t V0() const { return run0 >= 0 ? nv(g0()) : 0; }
  uint64_t E0() const { return run0 >= 0 ? ne(g0()) : 0; }
};

// nemo_set_option's values.  They outlive loads; some take effect at the next load only.
struct Options {
  uint32_t hcap_limit = 0xFFFFFFFFu, comp_limit = 0xFFFFFFFFu, build_limit = 0xFFFFFFFFu;
  uint32_t lds_limit = 0xFFFFFFFFu;  // test knob: largest V of the LDS graph tier (0 = off)
  uint64_t glob_min_v = 65536;       // graphs with V >= this take k_chains_glob (set before load)
  uint32_t gblock_force = 0;         // global_block option (0 = by corpus shape)
  uint32_t glob_block_force = 0;     // chains_glob_block option (0 = by the number of deep graphs)
  bool glob_prep_off = false;        // chains_glob_prep option 0: k_chains_glob builds its own H* order (test knob)
  bool topo_ell_off = true;          // topo_ell option 1: deep graphs' Kahn levels by k_topo_ell (measured slower
                                     // at C5: 103 vs 84 ms per launch with its records; kept as an option, tested)
  bool relax_off = true;             // option build_relax 1: k_build's Kahn levels by relaxation sweeps first
                                     // (measured slower at C3: k_build 2.96 -> 3.20 ms; kept as an option, tested)
  bool ms_fuse_off = true;           // option build_marksimp 1: k_build's marksimp tail (measured slower at C3:
                                     // k_build 3.00 -> 3.86 ms against k_marksimp's 0.80 ms; four workgroups
                                     // per CU by k_build's LDS image where k_marksimp runs eight waves per SIMD)
  uint32_t load_parts = 4;           // big-graph corpora upload in this many parts (nemo_load_corpus)
  bool load_async = false;           // nemo_load_corpus returns once its work is queued
  bool diff_on_aux = true;           // diff kernels on `aux` beside the simplification (option diff_aux)
  int diff_legacy = 0;               // one workgroup per entry (k_diff.hip)
  uint32_t diff_window = 0;          // test knob: 0 by size, 1 windowed, 2 tiny windows
  uint32_t diff_unfused = 0;         // option diff_fuse 0 (test knob): whole-graph walks hand LP rules to k_dx_lp / k_dx_emit
  // the simplified pull on `aux` (option pull_aux 1; off by default: beside k_proto_lds it made
  // the C3 step 8.3 -> 9.0 ms)
  uint32_t pull_on_aux = 0;
  uint32_t stage_on_aux = 1;  // the hand-over kernels of nemo_stage_simplified on `aux` (option stage_aux)
  uint32_t stage_blocks = 0;  // bulk staging: 0 = runtime copies, else k_to_host on this many blocks
  // nemo_stage_simplified packs and copies the node state in stage_slices slices, each stage_ratio times
  // the one before, and the chain pairs in stage_pair_slices equal slices; each slice's copy behind that
  // slice's kernel only (1: one kernel and one copy)
  uint32_t stage_slices = NEMO_STAGE_SLICES_DEFAULT, stage_ratio = NEMO_STAGE_RATIO_DEFAULT;
  uint32_t stage_pair_slices = NEMO_STAGE_PAIR_SLICES_DEFAULT;
  bool stage_sdma = false;    // runtime copies requested as NoCU (SDMA) copies (cleared if the runtime refuses)
  uint32_t stage_cus = 8;     // CUs of the copy stream (hipExtStreamCreateWithCUMask); 0 = unmasked
  int class_hash_bits = 128;  // nemo_diff_classes buckets by the low k bits of the hash (test knob: forces collisions)
  bool graph_dedup = true;    // option graph_dedup: the per-graph kernels run on one graph per distinct content
  int dedup_hash_bits = 128;  // the load's duplicate classes bucket by the low k bits of the hash (test knob)
  bool proto_dedup = true;    // option proto_dedup: k_proto_lds runs on one run per run class (with graph_dedup)
  bool replicate_lazy = true;  // option replicate_lazy: k_build's slices reach the duplicates when something reads them
  bool pull_dedup = true;     // option pull_dedup: raw / simplified pulls compact one graph per class (with graph_dedup)
  uint32_t pair_hash_lds_max = LAB_HASH_LDS_SLOTS;  // largest label table (slots) k_lab_hash builds in LDS (0: none)
  uint32_t near_bits_lds_max = NEAR_LDS_MAX;  // largest bit row (bytes) k_near_bits builds in LDS (0: none)
  uint32_t near_ksplit = 0;                   // k_near_isect's K ranges (0: by the tile count and the device)
  uint32_t knock_lds_max = KO_LDS_MAX;        // largest LDS image (bytes) k_ko_lds takes (0: every graph to k_ko_glob)
  uint32_t cut_grid = 0;                      // test knob: most workgroups of k_cut_lds / k_cut_glob (0: as many as are resident)
  bool kl_hitlist = true;                     // option kl_hitlist 0: k_kl_lds probes every node's label per chunk (the measured alternative)
  uint32_t kl_grid = 0;                       // test knob: most workgroups of k_kl_lds / k_kl_glob (0: as many as are resident)
  uint32_t wit_lds_max = WIT_LDS_DEFAULT;     // largest LDS image (bytes) k_wit_lds / k_lin_lds take (0: every graph to k_wit_glob / k_lin_glob)
  uint64_t lin_children_max = LIN_CHILDREN_DEFAULT;  // most children a level of nemo_lineage_cuts may emit (option lineage_children_max)
};

// Everything that belongs to the loaded corpus; release_corpus assigns CorpusState{}, so a member's
// default initialiser is its value with no corpus loaded.  Device pointers point into nemo_ctx::allocs.
struct CorpusState : GraphSizes {
  // host view (the graph offsets and run0 are GraphSizes')
  bool loaded = false, marked = false, simplified = false, protos_done = false;
  uint32_t n_runs = 0, G = 0, T = 0, W = 0, table_pre = 0, table_post = 0;
  uint64_t V = 0, E = 0;
  std::vector<uint32_t> iteration;
  std::vector<uint8_t> owned;
  std::unordered_map<uint32_t, uint32_t> it2run;
  bool has_rank = false;
  bool pairs_wide = false;           // some graph has >= 65536 nodes: u32 chain pairs
  double tierV = 0, tierE = 0;       // nodes / edges of the graphs within the tier's V/E caps
  uint32_t ms_rest = 0, pull_rest = 0;  // graphs past k_marksimp's / k_pull_lds's tiers (their global grids skipped at 0)
  double postV = 0, postE = 0;       // nodes / edges of the post graphs (k_proto's input)
  double bigV = 0, bigE = 0;         // nodes / edges of the graphs of >= NEMO_CSR_BIG nodes
  uint64_t bigVmax = 0;              // the largest of them
  uint32_t big_chunks = 1;           // k_csrb_* workgroups per big graph
  std::vector<uint32_t> big_host;    // the big-graph list (DevCorpus::big) on the host
  bool load_check_pending = false;   // option load_async: the graph checks wait for the next call that reads the graphs
  bool mark_pending = false;         // holds flags of the tier graphs not yet computed
  bool ms_fused = false;             // k_build's tail wrote its graphs' final flags at the last load / rebuild,
                                     // not yet consumed by nemo_simplify (k_marksimp skips those graphs)

  DevCorpus dc{};
  uint8_t *d_owned = nullptr, *d_is_success = nullptr;
  uint32_t *d_red = nullptr;
  const uint32_t *red_staged = nullptr;  // nemo_protos_stage's vector, copied into h_red behind ev_red

  // The global tiers' worklist sizes [load (k_csr/k_topo), chains (k_chains_list/_big), protos
  // (k_pg_*)] of the last full pass.  They are functions of the loaded corpus and the options
  // alone (sizes, Kahn level counts, in-degree caps, chain counts: every pass recomputes the
  // same), so once a pass's counts are known an empty tier is not launched at all (each of its
  // ~10 empty launches cost ~6 us on the analysis stream).  Reset by a load and by any option.
  bool tiers_pending = false, tiers_ok = false;
  uint32_t tiers[3] = {0, 0, 0}, tiers_run = 0;

  // Duplicate graphs (k_gdedup.hip, gdedup_host.h): classes of identical content, found once per
  // load (the inputs do not change until the next load; nemo_rebuild keeps them).  dc.dd_list is
  // d_gd_list while the option graph_dedup is on and the load found a duplicate, else null.
  std::vector<uint32_t> gd_rep;      // [G] graph -> its representative (empty: the load made no classes)
  uint32_t gd_nlist = 0, gd_npairs = 0, gd_classes = 0, gd_rounds = 0;
  uint32_t *d_gd_list = nullptr;     // [gd_nlist] the representatives
  uint32_t *d_gd_pairs = nullptr;    // [2 gd_npairs] (dup, rep) sorted by rep
  uint32_t *d_gd_rep = nullptr;      // [G] gd_rep on the device (DevCorpus::dd_rep)
  // k_build's slices of the duplicates (rp, rc, fp, fc, topo, lvl, nlv, e2, posoff) are not replicated yet:
  // set by a load / rebuild that deferred them, cleared by ensure_whole
  bool gd_stale = false;
  double gd_bytes[3] = {0, 0, 0};    // what a replicate pass writes per phase at most (timing table)
  // ... and the run classes (runs whose pre graphs are of one class and whose post graphs are): dc.run_list
  // is d_gd_rlist while dc.dd_list is set, the option proto_dedup is on and some run is a duplicate
  uint32_t gd_nrlist = 0, gd_nrpairs = 0;
  uint32_t *d_gd_rlist = nullptr;    // [gd_nrlist] the representative runs
  uint32_t *d_gd_rpairs = nullptr;   // [2 gd_nrpairs] (dup, rep) sorted by rep
  // ... and the raw / simplified pulls (option pull_dedup; gdedup::pull_plan): slot k of the launch is graph
  // pl.list[k] (d_pl_list), and graph g's (offset, count) is slot pl.map[g]'s (<= g).  The graphs past the
  // pull's LDS tier keep slots of their own, so the plan is made at the first pull under a tier (pl_tier)
  gdedup::PullPlan pl;
  Tier pl_tier{0, 0, 0, 0};
  bool pl_ok = false;
  DevBuf<uint32_t> d_pl_list;        // [G] the list | [n_big] the big graphs' slots
  double pl_V = 0, pl_E = 0;         // nodes / edges of the listed graphs (k_pull's timer, the capacity)

  // diff: per-call buffers in whole 64-entry chunks.  d_dsrc, d_dmask, d_miss grow together; so do the
  // one-workgroup-per-entry kernels' scratch d_dbits, d_dumask, d_ddepth, d_dtopo
  uint32_t n_entries = 0;
  uint32_t *d_r0lab = nullptr, *d_r0idx = nullptr, n_r0lab = 0;
  uint32_t *d_r0hkey = nullptr, *d_r0hval = nullptr, r0hmask = 0;
  uint32_t *d_r0dense = nullptr, nlab = 0;  // the dense label table of the multi-entry diff (DxArgs::r0dense)
  DevBuf<uint32_t> d_dsrc, d_miss, d_nmiss;
  DevBuf<uint8_t> d_dbits, d_dmask;
  DevBuf<int32_t> d_ddepth;
  DevBuf<uint32_t> d_dtopo;          // g0 in Kahn order (DiffArgs::tpos ...)
  uint64_t mrows_staged = 0;         // missing rows copied with the D masks
  // entries that share a label source share one computation: n_uniq distinct
  // sources, entry e's result is unique result dmap[e] (d_dmap on the device)
  uint32_t n_uniq = 0, *d_dmap = nullptr;  // (d_dmap points into d_dsrc)
  DevBuf<uint8_t> d_dumask;          // [n_uniq * V0] when n_uniq < n_entries
  std::vector<uint32_t> dmap;
  bool aux_pending = false;          // diff kernels queued on `aux` that `stream` has not joined (join_aux)
  // the multi-entry diff (k_dx.hip): g0's Kahn-order relayout, built with the
  // CSR in every load / rebuild, and the per-call buffers (grow-only)
  nemo::DxPrep dxp{};
  nemo::DxImg dx_img[2]{};           // walk images of g0 (k_dx.hip), built for the test knob dx_img_key
  nemo::DxImgScratch dx_its{};
  int dx_img_key = -1;               // -1: not built for the current load
  bool dx_ok = false;                // relayout allocated: run 0 present, every row fits a window
  uint32_t g0_maxdeg = 0;
  uint32_t dx_nu_cap = 0;            // sources the five buffers below hold (whole chunks); wflag's offset in d_dxlpl
  DevBuf<uint32_t> d_dxpb, d_dxsval, d_dxlpl, d_dxfb;
  DevBuf<uint64_t> d_dxw;  // [4][nch][V0] Good / LP, B, D, leaf candidates
  bool dx_last = false;              // the last diffprov ran the multi-entry kernels
  DevBuf<uint32_t> d_hlab;           // nemo_diffprov_host_labels' set [n, label...]

  // failure classes (k_dclass.hip): results of the last nemo_diff_classes, void after the next
  // diffprov / rebuild; buffers grow only, per-source sizes in whole 64-source chunks
  bool diff_done = false;            // a diffprov completed on the loaded corpus (n_entries may be 0)
  bool dc_done = false;
  hipStream_t diff_stream = nullptr;  // the stream the last diffprov's kernels went on (`aux` or the context's)
  uint32_t dc_cap = 0;               // sources the buffers hold; the offset of |D| and of the support in d_dcacc
  DevBuf<uint32_t> d_dcacc;          // [4 cap] hashes | [cap] |D| | [V0] support: zeroed, then summed into
  DevBuf<uint32_t> d_dcin;           // [2 cap] the sources' entry counts, then a round's (row, candidate) pairs
  DevBuf<uint8_t> d_dcv;             // [cap] a round's verdicts
  std::vector<uint32_t> dc_class_of;
  std::vector<nemo_diff_class> dc_classes;
  std::vector<dclass::Hash> dc_hash;  // per class: its mask's hash (the node context merges shards by it)
  std::vector<uint32_t> dc_support;  // [V0]
  uint32_t dc_rounds = 0;            // comparison rounds the last call took

  // symmetric diff (k_sdiff.hip): all of it the call's own state, so that a symmetric call leaves
  // the results of a previous nemo_diffprov alone and the reverse; buffers grow only
  bool sd_done = false;              // a symmetric call completed on the loaded corpus (n_sentries may be 0)
  uint32_t n_sentries = 0;
  std::vector<uint32_t> sd_graph;    // entry -> its failed post graph
  std::vector<uint64_t> sd_off;      // [n + 1] entry -> first node of its slices
  DevBuf<uint32_t> d_sdgraph;        // per entry, in whole 64-entry chunks; grows with d_sdoff
  DevBuf<uint64_t> d_sdoff;
  // the ragged buffers, exactly the largest node total so far: d_sdmask, d_sddepth, d_sdrows grow together;
  // d_sdbits (the global tier's node bits, as many as d_sdmask) is dropped with them and comes back only
  // for a call with a global-tier entry
  DevBuf<uint8_t> d_sdmask, d_sdbits;
  DevBuf<int32_t> d_sddepth;
  DevBuf<uint32_t> d_sdrows, d_sdn;
  // nemo_diffprov_pairs (the same state, and): the entries' and the tables' descriptors, and the
  // per-call region k_lab_hash builds the `other` runs' label tables in (pairs_host.h); grow only
  DevBuf<nemo::LabTab> d_sdtab;      // [2 x entries in whole chunks] entry -> its table, then the tables of the call
  std::vector<nemo::LabTab> sd_tabs;  // the last call's upload
  DevBuf<uint32_t> d_phreg;          // u32 slots, exactly the largest request so far

  // nearest runs (k_near.hip): the call's own state, void after the next call or load; independent of every
  // diff state.  near_lmax is the load's (found at the first call); the five buffers grow together, only inside
  // nemo_nearest_runs, in this order
  bool near_lmax_done = false, near_done = false;
  uint32_t near_lmax = 0, near_nq = 0, near_nc = 0;
  DevBuf<uint32_t> d_nrlmax;         // [1]
  DevBuf<uint64_t> d_nrbits;         // [rows][W]
  DevBuf<uint32_t> d_nrsize;         // [rows]
  DevBuf<uint32_t> d_nrmat;          // [n_q][n_c] intersections, then distances
  DevBuf<uint32_t> d_nrout;          // [n_q][4] nemo_nearest rows
  DevBuf<uint32_t> d_nrdesc;         // [rows] post graphs | [n_q] query rows | [n_c] candidate rows
  std::vector<uint32_t> nr_desc;     // the last call's upload

  // knock-out (k_knock.hip): the call's own state, void after the next call or load; independent of every diff,
  // nearest and class state.  d_kocnt grows alone, before the leaves are counted; the other five grow together
  // once the hypotheses are known, in this order; all of it only inside the two calls
  bool ko_done = false, ko_masks = false;
  knock::Table ko_tab;               // the last call's chunk table and ranges
  std::vector<uint32_t> ko_desc;     // the last leaves call's upload: [n] graphs | [n + 1] first hypotheses
  std::vector<uint64_t> ko_setoff;   // the last sets call's upload: set offsets from the first set's
  DevBuf<uint32_t> d_kocnt;          // [n] listed graphs | [n + 1] first hypotheses | [2 n] (leaves, Kahn levels)
  DevBuf<uint32_t> d_koleaf;         // [hypotheses] the leaf of each (leaves mode) / the sets' nodes (sets mode)
  DevBuf<knock::Chunk> d_kochunk;    // [chunks], then the two tiers' chunk lists (u32)
  DevBuf<uint64_t> d_koset;          // [sets + 1] set offsets into d_koleaf (sets mode)
  DevBuf<uint32_t> d_korows;         // [hypotheses][5] nemo_knock rows
  DevBuf<uint64_t> d_kodead;         // dead words of the chunks that keep them (knock::Chunk::moff)

  // minimal cut sets (k_cuts.hip): the call's own state, void after the next nemo_min_cuts or load; independent of
  // knock-out, diff, nearest and class state.  d_cutdesc grows alone inside nemo_min_cuts, behind a wait for the
  // stream, before anything is counted; cut.cand alone once the candidates are counted; the rest as CutBufs states
  CutBufs cut;                       // the search's (rows in nemo_ctx::h_cuts)
  uint64_t cut_stats[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // per size: live candidates, hypotheses, minimal cuts
  uint32_t cut_up[4] = {0, 0, 0, 0};  // the last call's uploads to d_cutdesc
  DevBuf<uint32_t> d_cutdesc;        // [8] k_ko_leaves' list, offsets and counts for the one graph (cand == NULL)

  // minimal repair sets (k_repair.hip): the two calls' own state, void after the next of them or a load; independent
  // of every other call's state.  Each buffer grows only inside the two calls, to the largest request so far, behind a
  // wait for the stream: rp_abs as AbsentSet states, its bitmap together with rp.cand; the rest as CutBufs states
  CutBufs rp;                        // the search's (rows in nemo_ctx::h_repair); w[0]: round 0's word behind round 1's
  uint64_t rp_stats[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // status, |A|, then per size: live candidates, hypotheses, minimal repairs
  AbsentSet rp_abs;                  // the absent set (repair_api.h)

  // knock-out by label (k_klabel.hip): the call's own state, void after the next nemo_knockout_labels or load;
  // independent of knock-out, cut, diff, nearest and class state.  The eight buffers grow as one group, only
  // inside nemo_knockout_labels, each to the largest request so far, behind a wait for the stream, in this order
  bool kl_done = false;
  uint64_t kl_n = 0, kl_sets = 0, kl_chunks = 0;  // list positions, sets and chunks of the last call
  std::vector<uint32_t> kl_nlev;     // [G] the graphs' Kahn level counts (the tier), read once per load
  std::vector<uint64_t> kl_setoff;   // the last call's uploads: set offsets from the first set's,
  std::vector<uint64_t> kl_taboff;   // ... the tables' first slots,
  std::vector<uint32_t> kl_desc;     // ... [n] graphs | the LDS tier's list positions | the global tier's
  DevBuf<uint64_t> d_klset;          // [sets + 1]
  DevBuf<uint32_t> d_kllab;          // the sets' labels
  DevBuf<uint64_t> d_kltoff;         // [chunks + 2]
  DevBuf<uint32_t> d_klkey;          // the tables' keys: per chunk, then the union filter
  DevBuf<uint64_t> d_klmask;         // ... and masks
  DevBuf<uint32_t> d_kldesc;         // [2 n]
  DevBuf<uint64_t> d_klout;          // [n][chunks][2] (lost, hit), then the counts (u32: [chunks * 64] lost | hit)
  DevBuf<uint64_t> d_klreg;          // the workgroups' regions: hit-list spill, k_kl_glob's dead words

  // minimal cut sets by label (k_lcuts.hip): the call's own state, void after the next nemo_min_label_cuts or load;
  // independent of knock-out, cut, label knock-out, diff, nearest and class state (kl_nlev above is the load's, not
  // a result).  All of it grows only inside nemo_min_label_cuts, each buffer to the largest request so far, behind
  // a wait for the stream: the first ten together once the call is checked, in this order; d_lcw[1..2],
  // d_lclost[1..2] and d_lcscan together once round 1 has left the live list; d_lcrows alone once the totals are known
  bool lc_done = false;
  uint64_t lc_rows = 0;              // rows of the last call (in nemo_ctx::h_lcuts: [rows][4], then [rows] n_lost)
  uint64_t lc_stats[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // per size: live candidates, hypotheses, minimal cuts
  std::vector<uint32_t> lc_desc;     // the last call's uploads: [n] graphs | the LDS tier's list positions | the global tier's,
  std::vector<uint32_t> lc_map;      // ... [K] candidate position -> live position (round 1's, then the later rounds'),
  std::vector<uint32_t> lc_live;     // ... [K1] live position -> candidate position
  DevBuf<uint32_t> d_lccand;         // [K] candidate position -> label
  DevBuf<uint32_t> d_lcmap;          // [2 K] round 1's map (the identity) | the later rounds'
  DevBuf<uint32_t> d_lclive;         // [K]
  DevBuf<uint32_t> d_lckey;          // the table's keys
  DevBuf<uint32_t> d_lcval;          // ... and candidate positions
  DevBuf<uint32_t> d_lcdesc;         // [2 n]
  DevBuf<uint64_t> d_lchit;          // [n][chunks] round 1's hit words
  DevBuf<uint64_t> d_lcreg;          // the workgroups' regions: the hit list's rest, k_lc_glob's dead words
  DevBuf<uint64_t> d_lcw[3];         // the rounds' cut words, one per chunk of 64 ranks (round 1: then the any-hit words)
  DevBuf<uint64_t> d_lclost[3];      // the rounds' lost words [n][chunks]
  DevBuf<uint32_t> d_lcscan;         // per round [chunks + 1] popcounts -> first rows; then the scan's tile sums
  DevBuf<uint32_t> d_lcrows;         // [rows][4] nemo_label_cut, then [rows] n_lost

  // minimal cut sets over fault events (k_gcuts.hip): the call's own state, void after the next nemo_min_group_cuts or
  // load; independent of knock-out, cut, label knock-out, label cut, diff, nearest and class state (kl_nlev above is
  // the load's, not a result).  One group d_gc*, which grows only inside nemo_min_group_cuts, each buffer to the
  // largest request so far, behind a wait for the stream: the first eleven together once the call is checked, in this
  // order; d_gcw[1..2], d_gclost[1..2] and d_gcscan together once round 1 has left the live list; d_gcrows alone once
  // the totals are known
  bool gc_done = false;
  uint64_t gc_rows = 0;              // rows of the last call (in nemo_ctx::h_gcuts: [rows][4], then [rows] n_lost)
  uint64_t gc_stats[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // per size: live candidates, hypotheses, minimal cuts
  std::vector<uint32_t> gc_desc;     // the last call's uploads: [n] graphs | the LDS tier's list positions | the global tier's,
  std::vector<uint32_t> gc_off;      // ... [K + 1] the groups' offsets from the first group's,
  std::vector<uint32_t> gc_ident;    // ... [K] the identity (a row's entries are candidate positions),
  std::vector<uint32_t> gc_live;     // ... [K1] live position -> candidate position
  DevBuf<uint32_t> d_gcoff;          // [K + 1]
  DevBuf<uint32_t> d_gcgrow;         // the groups' labels, rewritten as rows
  DevBuf<uint32_t> d_gcident;        // [K]
  DevBuf<uint32_t> d_gclive;         // [K]
  DevBuf<uint32_t> d_gckey;          // the table's keys; then the rows handed out (one word)
  DevBuf<uint32_t> d_gcval;          // ... and rows
  DevBuf<uint32_t> d_gcdesc;         // [2 n]
  DevBuf<uint64_t> d_gchit;          // [n][chunks] round 1's hit words
  DevBuf<uint64_t> d_gcreg;          // the workgroups' regions: the hit list's rest, k_gc_glob's dead words
  DevBuf<uint64_t> d_gcw[3];         // the rounds' cut words, one per chunk of 64 ranks (round 1: then the any-hit words)
  DevBuf<uint64_t> d_gclost[3];      // the rounds' lost words [n][chunks]
  DevBuf<uint32_t> d_gcscan;         // per round [chunks + 1] popcounts -> first rows; then the scan's tile sums
  DevBuf<uint32_t> d_gcrows;         // [rows][4] nemo_group_cut, then [rows] n_lost

  // surviving derivations (k_witness.hip): the two witness calls' own state, void after the next witness call or load;
  // independent of knock-out, cut, label knock-out, label cut, group cut, diff, nearest and class state (kl_nlev above
  // is the load's, not a result).  One group d_wt*, which grows only inside the two calls, each buffer to the largest
  // request so far, behind a wait for the stream, in this order
  bool wit_done = false, wit_masks = false;
  uint64_t wit_n = 0, wit_sets = 0, wit_chunks = 0;  // list positions, sets and chunks of the last call
  std::vector<uint32_t> wit_desc;    // the last call's uploads: [n] graphs | the LDS tier's list positions | the global tier's,
  std::vector<uint64_t> wit_setoff;  // ... set offsets from the first set's,
  std::vector<uint32_t> wit_ent;     // ... the label form's entries as rows, then the distinct labels,
  std::vector<uint64_t> wit_moff;    // ... [n] list position -> its first kept need word
  DevBuf<uint64_t> d_wtset;          // [sets + 1]
  DevBuf<uint32_t> d_wtent;          // the sets' entries (nodes / rows), then the distinct labels
  DevBuf<uint32_t> d_wtkey;          // the table's keys
  DevBuf<uint32_t> d_wtval;          // ... and rows
  DevBuf<uint32_t> d_wtdesc;         // [2 n]
  DevBuf<uint64_t> d_wtmoff;         // [n]
  DevBuf<uint32_t> d_wtrows;         // [n][sets][5] nemo_witness
  DevBuf<uint64_t> d_wtneed;         // the kept need words (NEMO_WIT_MASKS)
  DevBuf<uint64_t> d_wtreg;          // the workgroups' regions: k_wit_glob's dead and need words, the hit list's rest

  // lineage-driven cut search (k_lineage.hip): the call's own state, void after the next nemo_lineage_cuts or load;
  // independent of every other call's state (kl_nlev above is the load's, not a result).  One group d_ln*, which grows
  // only inside nemo_lineage_cuts, each buffer to the largest request so far, behind a wait for the stream: d_lndesc
  // alone, before anything is counted; d_lncand alone once the candidates are counted; d_ln.ctr and d_lnreg together
  // once the tier is known (lin_api.h's lin_node_search), in this order; the rest of d_ln as LinBufs states
  bool lin_done = false;
  uint64_t lin_stats[18] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // per size 0..8: sets evaluated, minimal cuts
  std::vector<nemo_lineage_cut> lin_rows;  // the last call's rows, sorted
  std::vector<uint32_t> lin_cand;    // the last call's candidates (nodes)
  uint32_t lin_up[4] = {0, 0, 0, 0};  // the last call's uploads to d_lndesc
  DevBuf<uint32_t> d_lndesc;         // [8] k_ko_leaves' list, offsets and counts for the one graph (cand == NULL)
  DevBuf<uint32_t> d_lncand;         // [K] candidate position -> node
  DevBuf<uint64_t> d_lnreg;          // k_lin_glob: dead and need words of every workgroup of the launch
  LinBufs d_ln;                      // the level loop's

  // lineage cut search over fault events (k_lgcuts.hip): the call's own state, void after the next
  // nemo_lineage_group_cuts or load; independent of every other call's state (kl_nlev above is the load's, not a
  // result).  One group d_lg*, which grows only inside nemo_lineage_group_cuts, each buffer to the largest request so
  // far, behind a wait for the stream: the first five, d_lg.ctr and d_lgreg together once the call is checked, in this
  // order; d_lglost alone before a level of more chunks; the rest of d_lg as LinBufs states, d_lgnl, its counts kept,
  // alongside d_lg.cuts
  bool lg_done = false;
  uint64_t lg_stats[18] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // per size 0..8: sets evaluated, minimal cuts
  std::vector<nemo_lineage_group_cut> lg_rows;  // the last call's rows, sorted,
  std::vector<uint32_t> lg_nlost;    // ... and their lost counts
  std::vector<uint32_t> lg_desc;     // the last call's uploads: [n] graphs | the LDS tier's list positions | the global tier's,
  std::vector<uint32_t> lg_off;      // ... [K + 1] the groups' offsets from the first group's
  DevBuf<uint32_t> d_lgoff;          // [K + 1]
  DevBuf<uint32_t> d_lggrow;         // the groups' labels, rewritten as rows
  DevBuf<uint32_t> d_lgkey;          // the table's keys; then the rows handed out (one word)
  DevBuf<uint32_t> d_lgval;          // ... and rows
  DevBuf<uint32_t> d_lgdesc;         // [2 n]
  DevBuf<uint64_t> d_lgreg;          // the workgroups' regions: k_lgc_glob's dead and need words, the rows' need words, the hit list's rest
  DevBuf<uint64_t> d_lglost;         // [n][chunks] a level's lost words
  LinBufs d_lg;                      // the level loop's
  DevBuf<uint32_t> d_lgnl;           // [cap] the cuts' lost counts

  // lineage repair search (k_lrepair.hip): the two calls' own state, void after the next nemo_lineage_repair_sets /
  // nemo_lineage_repairs or load; independent of every other call's state (kl_nlev above is the load's, not a result).
  // One group, which grows only inside the two calls, each buffer to the largest request so far, behind a wait for the
  // stream: lr_abs as AbsentSet states, its bitmap together with d_lrcand; d_lr.ctr and d_lrreg together once the tier
  // is known (lin_api.h's lin_node_search), in this order; the rest of d_lr as LinBufs states
  bool lr_done = false;
  uint64_t lr_stats[20] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // status, |A|, then per size 0..8: sets evaluated, minimal repairs
  std::vector<nemo_lineage_repair> lr_rows;  // the last call's rows, sorted
  std::vector<uint32_t> lr_cand;     // the last call's candidates (nodes)
  AbsentSet lr_abs;                  // the absent set (repair_api.h)
  DevBuf<uint32_t> d_lrcand;         // [K] candidate position -> node
  DevBuf<uint64_t> d_lrreg;          // k_lrep_glob: dead, blame and stop-rule words of every workgroup of the launch
  LinBufs d_lr;                      // the level loop's; ctr[3]: the two-hypothesis launch's lost word

  // pulls: per-slot (offset, count) and the region cursor come back to pinned
  // memory asynchronously; the first fetch waits for them
  int pull_which = -1;
  uint32_t pull_slots = 0;
  uint32_t pull_dslots = 0;              // slots computed: diff entries sharing a label source share one
  std::vector<uint32_t> pull_map;        // which 2 with shared slots: entry -> computed slot
  // the map pull_sync expands the slot tables by, once (null: none, or done): pull_map's, or pl.map's
  // for a raw / simplified pull over one graph per class
  const uint32_t *pull_expand = nullptr;
  DevBuf<uint32_t> d_pck;             // big graphs' pull chunk table
  DevBuf<uint32_t> d_pcnt;            // the slot tables: d_pcnt and d_poff grow together
  DevBuf<uint64_t> d_poff;
  // the regions: d_psrc and d_pdst grow together (pull_grow); d_pdst, allocated last, has the pull's
  // capacity in edges (PullArgs::cap)
  DevBuf<uint32_t> d_psrc, d_pdst;
  DevBuf<unsigned long long> d_pcur;
  bool pull_synced = true;
  bool pull_aux_pending = false;      // a pull on `aux` not yet joined by `stream` (guard_staged)
  uint64_t pull_hint[4] = {0, 0, 0, 0};
  nemo::PullArgs pull_args{};

  // triggers: outputs sized at load from run 0's degrees (exact bounds), one
  // launch; the row counts come back to pinned memory asynchronously
  bool trig_done = false, trig_pending = false;
  DevBuf<uint32_t> d_tcounts;
  uint32_t *d_tpre = nullptr, *d_tpost = nullptr, *d_tasync = nullptr;  // (the load's)
  uint32_t tcounts[3] = {0, 0, 0};
  uint64_t tcap[3] = {0, 0, 0};

  // chain gather
  DevBuf<uint32_t> d_chout;  // 5 words per chain
  DevBuf<uint64_t> d_choff;

  // staged simplification results
  bool flags_final = false;  // ev_flags marks the current flags (no flag-rewriting call since)
  bool chains_final = false;  // ev_simp marks the current chain and nch (nothing that may rewrite them since)
  hipStream_t stage_stream = nullptr;  // the stream the last stage's hand-over kernels went on
  bool staged = false;
  uint64_t staged_n = 0, staged_cap = 0, chht_hint = 0;
  DevBuf<uint32_t> d_state;  // 2-bit node state (k_pack_state)
  DevBuf<uint32_t> d_chht;   // the staged chain pairs and two words of padding
};

struct nemo_ctx {
  Node *node = nullptr;  // node context: every entry point dispatches to node.hip
  int device = 0;
  Options opt;
  CorpusState cs;
  std::string err;

  // streams: `stream` is the caller's (nemo_set_stream) or `own`; the others are created at first use
  hipStream_t own = nullptr, stream = nullptr;
  // uploads of a corpus of big graphs, in parts, so that the CSR build of part k overlaps the
  // upload of part k + 1 (nemo_load_corpus; option load_parts)
  hipStream_t up = nullptr;
  // CreateNaiveDiffProv reads only the raw run-0 graph and the label sources
  // (differential-provenance.go:22-98), so its kernels run on `aux`, beside
  // the simplification on `stream`; whatever rewrites the graphs' structure,
  // or reads the D masks on `stream`, first waits for ev_diff (join_aux)
  hipStream_t aux = nullptr;
  hipStream_t copy = nullptr;  // staged simplification results: pinned host copies made on `copy`
  hipStream_t *const streams[4] = {&copy, &up, &aux, &own};  // the context's own, in nemo_ctx_destroy's order

  // named events, created by ensure_event at first use
  hipEvent_t ev_fork = nullptr, ev_pull = nullptr, ev_trig = nullptr;
  hipEvent_t ev_protos = nullptr, ev_red = nullptr, ev_diff = nullptr, ev_misc = nullptr, ev_tiers = nullptr;
  // pinned upload staging is reused once the previous upload from the same buffer has landed
  hipEvent_t ev_up_hlab = nullptr, ev_up_succ = nullptr, ev_up_dsrc = nullptr;
  // one per slice of the chain pairs (stage_pair_slices): the slice's pairs are on the device
  hipEvent_t ev_ready[NEMO_STAGE_SLICES_MAX] = {};
  hipEvent_t ev_copied = nullptr;  // the last slice's copy has landed: behind every other copy of the stage
  // a simplified pull on `aux` waits for the end of nemo_simplify (ev_simp) only, so it runs
  // beside the protos and hand-over kernels of `stream`; anything that rewrites its inputs
  // first waits for ev_auxpull
  hipEvent_t ev_simp = nullptr, ev_auxpull = nullptr;
  // recorded by nemo_simplify once the node flags are final (after the mark / clean / delete-set
  // kernels, before the chain cover, which only reads them): the staged 2-bit node state is
  // packed and copied from there on, beside the chain cover (nemo_stage_simplified)
  // (ev_state: one per slice of the state, recorded behind the slice's k_pack_state)
  hipEvent_t ev_flags = nullptr, ev_state[NEMO_STAGE_SLICES_MAX] = {};
  // the hand-over kernels of nemo_stage_simplified on `aux`: behind everything `stream` has
  // queued so far, beside the triggers and pulls queued after
  hipEvent_t ev_stage = nullptr;
  hipEvent_t ev_dclass = nullptr;  // nemo_diff_classes' hashes / verdicts have reached pinned memory
  hipEvent_t ev_near = nullptr;    // nemo_nearest_runs' label maximum / rows have reached pinned memory
  hipEvent_t ev_whole = nullptr;   // ensure_whole's replicate is queued on `stream`: `aux` waits for it
  hipEvent_t ev_knock = nullptr;   // the knock-out calls' counts / rows have reached pinned memory
  hipEvent_t ev_cuts = nullptr;    // nemo_min_cuts' counts / words / totals / rows have reached pinned memory
  hipEvent_t ev_klabel = nullptr;  // nemo_knockout_labels' level counts / words / counts have reached pinned memory
  hipEvent_t ev_lcuts = nullptr;   // nemo_min_label_cuts' level counts / round 1's words / totals / rows have reached pinned memory
  hipEvent_t ev_gcuts = nullptr;   // nemo_min_group_cuts' level counts / round 1's words / totals / rows have reached pinned memory
  hipEvent_t ev_wit = nullptr;     // the witness calls' level counts / rows have reached pinned memory
  hipEvent_t ev_lin = nullptr;     // nemo_lineage_cuts' counts / candidates / a level's counters / the cuts have reached pinned memory
  hipEvent_t ev_lgc = nullptr;     // nemo_lineage_group_cuts' level counts / a level's counters / the cuts have reached pinned memory
  hipEvent_t ev_repair = nullptr;  // the repair calls' counts / rounds 0 and 1's words / totals / rows have reached pinned memory
  hipEvent_t ev_lrep = nullptr;    // the lineage repair calls' counts / status word / a level's counters / the repairs have reached pinned memory
  hipEvent_t *const events[29] = {&ev_fork,    &ev_pull,    &ev_trig,  &ev_protos, &ev_red,  &ev_diff,
                                  &ev_misc,    &ev_tiers,   &ev_up_hlab, &ev_up_succ, &ev_up_dsrc,
                                  &ev_copied,  &ev_simp,    &ev_auxpull, &ev_flags, &ev_stage,
                                  &ev_dclass,  &ev_near,    &ev_whole,   &ev_knock,
                                  &ev_cuts,    &ev_klabel,  &ev_lcuts,   &ev_gcuts,
                                  &ev_wit,     &ev_lin,     &ev_lgc,     &ev_repair,
                                  &ev_lrep};
  // ... and the slices' (ev_state, ev_ready), destroyed with them
  std::vector<hipEvent_t> ev_up;  // one per upload part

  // pinned result hand-over, written by k_to_host (device -> pinned host), and upload staging
  Pinned<uint32_t> h_red, h_tab, h_nmiss, h_mrows, h_tpre, h_tpost, h_tasync, h_tcounts, h_tiers;
  Pinned<uint8_t> h_mask, h_succ, h_flags;
  Pinned<uint32_t> h_hlab, h_dsrc, h_chht;
  Pinned<uint64_t> h_choff;
  PullHost h_pull;
  // nemo_diff_classes: h_dcin uploads (entry counts, pairs), h_dcout receives (hashes, |D|, support, verdicts)
  Pinned<uint32_t> h_dcin, h_dcout;
  Pinned<uint32_t> h_near;  // nemo_nearest_runs: [n_q][4] rows, then the label maximum
  Pinned<uint32_t> h_knock;  // the knock-out calls: the listed graphs' (leaves, Kahn levels), then the rows
  Pinned<uint32_t> h_cuts;   // nemo_min_cuts: counts, round 1's words and the candidates, the totals, then the rows
  Pinned<uint64_t> h_klabel;  // nemo_knockout_labels: the level counts; then the (lost, hit) words and the counts
  Pinned<uint32_t> h_lcuts;  // nemo_min_label_cuts: the level counts, round 1's words, the totals; then the rows and their n_lost
  Pinned<uint32_t> h_gcuts;  // nemo_min_group_cuts: the level counts, round 1's words, the totals; then the rows and their n_lost
  Pinned<uint32_t> h_wit;    // the witness calls: the level counts; then the rows
  Pinned<uint64_t> h_lin;    // nemo_lineage_cuts: the level counts, the counts and candidates, a level's counters; then the cuts' keys
  Pinned<uint64_t> h_lgc;    // nemo_lineage_group_cuts: the level counts, a level's counters; then the cuts' keys and lost counts
  Pinned<uint32_t> h_repair;  // the repair calls: counts, rounds 0 and 1's words and the candidates, the totals, then the rows
  Pinned<uint64_t> h_lrep;   // the lineage repair calls: the level counts, the counts and candidates, the status word, a level's counters; then the repairs' keys
  void **const pinned[32] = {h_red.slot(),   h_tab.slot(),     h_nmiss.slot(), h_mrows.slot(), h_tpre.slot(),
                             h_tpost.slot(), h_tasync.slot(),  h_tcounts.slot(), h_tiers.slot(), h_mask.slot(),
                             h_succ.slot(),  h_flags.slot(),   h_hlab.slot(),  h_dsrc.slot(),  h_chht.slot(),
                             h_choff.slot(), h_pull.cnt.slot(), h_pull.off.slot(), h_pull.cur.slot(),
                             h_dcin.slot(),  h_dcout.slot(),   h_near.slot(),  h_knock.slot(),
                             h_cuts.slot(),  h_klabel.slot(), h_lcuts.slot(),
                             h_gcuts.slot(),  h_wit.slot(),    h_lin.slot(),   h_lgc.slot(),
                             h_repair.slot(),  h_lrep.slot()};
  // missing rows copied with the D masks: the last nemo_fetch_missing's count.  A size hint only
  // (a short one costs a second copy), kept across loads: batches of one shape find as many rows
  uint64_t mrows_hint = 256;

  // device blocks: `allocs` are the loaded corpus's, `cache` the previous corpus's, kept for the
  // next load (nemo_load_corpus frees what it did not reuse): reloading a corpus of the same
  // shape allocates nothing
  std::vector<void *> allocs;
  std::unordered_map<void *, size_t> alloc_bytes;  // every live allocation's size (allocs and the cache)
  std::multimap<size_t, void *> cache;
  // NEMO_LOAD_DEBUG: dalloc calls since the load began and a running hash of their sizes in order
  uint64_t dalloc_n = 0, dalloc_hash = 0;
  // ... and the per-call requests: dalloc / dfree calls since the last load finished, and the same hash over
  // their sizes in order (release_corpus prints them)
  uint64_t call_dalloc_n = 0, call_dfree_n = 0, call_hash = 0xCBF29CE484222325ull;

  // per-kernel timing
  std::vector<std::string> tgroups;  // nemo_set_timing_groups: the timed groups (empty: all)
  bool timing = false;
  std::vector<PendingEv> pending;
  std::vector<hipEvent_t> ev_pool;
  std::map<std::string, Agg> agg;
};

static inline int fail(nemo_ctx *c, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return code;
}

// the cached blocks (nemo_ctx::cache)
static inline void drop_cache(nemo_ctx *c) {
  for (auto &b : c->cache) {
    c->alloc_bytes.erase(b.second);
    hipFree(b.second);
  }
  c->cache.clear();
}

template <class T>
static int dalloc(nemo_ctx *c, T **p, size_t n) {
  void *q = nullptr;
  if (n == 0) n = 1;
  // whole 16-byte chunks: stage_lds (device.h) loads aligned 16-B chunks, so
  // the chunk holding a buffer's last byte must lie inside the allocation
  const size_t bytes = (n * sizeof(T) + 15) & ~(size_t)15;
  c->dalloc_n++;
  c->dalloc_hash = (c->dalloc_hash ^ bytes) * 0x100000001B3ull;  // the request order decides who gets which cached block
  c->call_dalloc_n++;
  c->call_hash = (c->call_hash ^ bytes) * 0x100000001B3ull;
  auto it = c->cache.lower_bound(bytes);  // the smallest cached block that fits, if not much larger
  if (it != c->cache.end() && it->first <= bytes + bytes / 8 + (1u << 20)) {
    q = it->second;
    c->cache.erase(it);
  } else {
    // large blocks get headroom, so that the next corpus of about the same shape reuses them: 1/16
    // (C5's 143-run batches differ by up to 3.3 % in edges; at 1/32 a load found some block too small
    // about every other time, allocated anew (~28 ms) and the next load's drop_cache freed the unused
    // block: hipFree waits for the whole device, ~220 ms behind the other context's analysis)
    const size_t want = bytes >= (64u << 20) ? ((bytes + bytes / 16) + (2u << 20) - 1) & ~(size_t)((2u << 20) - 1) : bytes;
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t e = hipMalloc(&q, want);
    if (getenv("NEMO_LOAD_DEBUG") && want >= (64u << 20))
      fprintf(stderr, "dalloc: new block %zu MB (%s) %.1f ms, %zu cached\n", want >> 20, e == hipSuccess ? "ok" : "failed",
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), c->cache.size());
    if (e != hipSuccess) {
      (void)hipGetLastError();
      drop_cache(c);  // no room: the cached blocks go first, then the headroom
      e = hipMalloc(&q, bytes);
      if (e != hipSuccess) return fail(c, NEMO_ERR_HIP, "hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
      c->alloc_bytes[q] = bytes;
    } else {
      c->alloc_bytes[q] = want;
    }
  }
  c->allocs.push_back(q);
  *p = (T *)q;
  return NEMO_OK;
}

static inline void dfree(nemo_ctx *c, void *p) {
  if (!p) return;
  auto it = std::find(c->allocs.begin(), c->allocs.end(), p);
  if (it != c->allocs.end()) c->allocs.erase(it);
  auto b = c->alloc_bytes.find(p);
  c->call_dfree_n++;
  c->call_hash = (c->call_hash ^ (b != c->alloc_bytes.end() ? b->second : 0)) * 0x100000001B3ull;
  c->alloc_bytes.erase(p);
  hipFree(p);
}

static inline hipEvent_t get_event(nemo_ctx *c) {
  if (!c->ev_pool.empty()) {
    hipEvent_t e = c->ev_pool.back();
    c->ev_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  hipEventCreate(&e);
  return e;
}

static inline int ensure_event(nemo_ctx *c, hipEvent_t *e) {
  if (!*e) HIPCHK(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
  return NEMO_OK;
}

// Kernels that rewrite node flags must not overtake a staged copy still in flight.
static inline int guard_staged(nemo_ctx *c) {
  c->cs.flags_final = false;  // the caller is about to rewrite node flags
  c->cs.chains_final = false;  // ... and the chains with them, or the graphs under them
  if (c->cs.staged) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_copied, 0));
  if (c->cs.pull_aux_pending) {  // a pull on `aux` still reads the graphs, flags and chains
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_auxpull, 0));
    c->cs.pull_aux_pending = false;
  }
  return NEMO_OK;
}

// the finished timed launches into `agg`; their events go back to the pool
static inline int collect_timings(nemo_ctx *c) {
  for (auto &p : c->pending) {
    HIPCHK(c, hipEventSynchronize(p.b));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, p.a, p.b));
    Agg &g = c->agg[p.name];
    g.launches++;
    g.ms += ms;
    g.bytes += p.bytes;
    g.edges += p.edges;
    c->ev_pool.push_back(p.a);
    c->ev_pool.push_back(p.b);
  }
  c->pending.clear();
  return NEMO_OK;
}

template <class F>
static int timed_on(nemo_ctx *c, hipStream_t st, const char *name, double bytes, double edges, F &&f) {
  hipEvent_t a = nullptr, b = nullptr;
  const bool timed = c->timing && (c->tgroups.empty() ||
                                   std::find(c->tgroups.begin(), c->tgroups.end(), name) != c->tgroups.end());
  if (timed) {
    a = get_event(c);
    b = get_event(c);
    hipEventRecord(a, st);
  }
  f();
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, NEMO_ERR_HIP, "launch %s: %s", name, hipGetErrorString(e));
  if (timed) {
    hipEventRecord(b, st);
    c->pending.push_back({name, a, b, bytes, edges});
    if (c->pending.size() > 4096) collect_timings(c);  // bound outstanding events (they may be on two streams)
  }
  return NEMO_OK;
}

template <class F>
static int timed(nemo_ctx *c, const char *name, double bytes, double edges, F &&f) {
  return timed_on(c, c->stream, name, bytes, edges, f);
}

// The outer timing group of a call (the knock-out family's: knock_api.h): every launch of the call between one pair
// of events, reported under `name`.
struct GroupTimer {
  nemo_ctx *c;
  const char *name;
  hipEvent_t ta = nullptr;
  GroupTimer(nemo_ctx *c_, const char *name_) : c(c_), name(name_) {
    const bool on = c->timing && (c->tgroups.empty() || std::find(c->tgroups.begin(), c->tgroups.end(), name) != c->tgroups.end());
    if (on) {
      ta = get_event(c);
      hipEventRecord(ta, c->stream);
    }
  }
  void done(double bytes, double ops) {
    if (!ta) return;
    hipEvent_t tb = get_event(c);
    hipEventRecord(tb, c->stream);
    c->pending.push_back({name, ta, tb, bytes, ops});
    ta = nullptr;
  }
  ~GroupTimer() {
    if (ta) c->ev_pool.push_back(ta);
  }
};

// `need` elements in each buffer of a group that grows together: each to the largest request so far, released
// together and allocated in the given order, behind a wait for the stream (an earlier launch may still read them)
template <class... B>
static int grow_group(nemo_ctx *c, const uint64_t *need, B &...bufs) {
  bool ok = true;
  int i = 0;
  ((ok = ok && bufs.p && need[i++] <= bufs.cap), ...);
  if (ok) return NEMO_OK;
  uint64_t cap[sizeof...(B)];
  i = 0;
  ((cap[i] = std::max<uint64_t>(need[i], bufs.cap), i++), ...);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  (bufs.release(c), ...);
  int rc = NEMO_OK;
  i = 0;
  ((rc = rc ? rc : bufs.grow(c, cap[i++])), ...);
  return rc;
}

// `stream` waits for the diff kernels queued on `aux` (see nemo_ctx::aux)
static inline int join_aux(nemo_ctx *c) {
  if (!c->cs.aux_pending) return NEMO_OK;
  HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_diff, 0));
  c->cs.aux_pending = false;
  return NEMO_OK;
}

static inline int run_index(nemo_ctx *c, uint32_t it, uint32_t *r) {
  auto f = c->cs.it2run.find(it);
  if (f == c->cs.it2run.end()) return fail(c, NEMO_ERR_NOTFOUND, "unknown run iteration %u", it);
  *r = f->second;
  return NEMO_OK;
}

template <int K>
static void sort_rows(uint32_t *rows, uint64_t n) {
  std::vector<std::array<uint32_t, K>> v(n);
  for (uint64_t i = 0; i < n; i++)
    for (int k = 0; k < K; k++) v[i][k] = rows[K * i + k];
  std::sort(v.begin(), v.end());
  for (uint64_t i = 0; i < n; i++)
    for (int k = 0; k < K; k++) rows[K * i + k] = v[i][k];
}

static inline int check_graph_errors(nemo_ctx *c) {
  std::vector<uint32_t> err(c->cs.G), created(c->cs.G);
  HIPCHK(c, hipMemcpyAsync(err.data(), c->cs.dc.err, c->cs.G * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(created.data(), c->cs.dc.created, c->cs.G * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (uint32_t g = 0; g < c->cs.G; g++) {
    if (!err[g]) continue;
    const uint32_t it = c->cs.iteration[g / 2];
    const uint64_t E = c->cs.ne(g);
    if (err[g] == NEMO_ERR_LOAD)
      return fail(c, NEMO_ERR_LOAD,
                  "Run %u: inserted number of edges (%u) does not equal number of antecedent provenance edges (%llu)",
                  it, created[g], (unsigned long long)E);
    if (err[g] == NEMO_ERR_CYCLE) return fail(c, NEMO_ERR_CYCLE, "Run %u: provenance graph is not acyclic", it);
    return fail(c, (int)err[g], "Run %u: edge references a node index out of range", it);
  }
  return NEMO_OK;
}

// Option load_async: the last load's graph checks (validations, acyclicity), before the first call
// that reads its graphs; a failed check leaves no corpus loaded, as a failed nemo_load_corpus does.
static inline int ensure_load_checked(nemo_ctx *c) {
  if (!c->cs.load_check_pending) return NEMO_OK;
  c->cs.load_check_pending = false;
  const int rc = check_graph_errors(c);
  if (rc) c->cs.loaded = false;
  return rc;
}

// Duplicate graphs, option replicate_lazy (DESIGN.md §3 "Duplicate graphs"): a load / rebuild whose pass
// is known to read the k_build slices of representatives only leaves the duplicates' slices stale.  Every
// entry point calls this first, except the ones that state at their call site which graphs' build outputs
// they read.  The replicate goes on `stream`; `aux`, where the diff kernels read graphs, waits for it.
static inline int ensure_whole(nemo_ctx *c) {
  if (!c->cs.gd_stale) return NEMO_OK;
  int rc = timed(c, "k_replicate", c->cs.gd_bytes[GD_BUILD], 0, [&] {
    nemo::launch_replicate(c->cs.dc, c->cs.d_gd_pairs, c->cs.gd_npairs, GD_BUILD_SLICES, c->stream);
  });
  if (rc) return rc;
  c->cs.gd_stale = false;
  if (c->aux) {
    if ((rc = ensure_event(c, &c->ev_whole))) return rc;
    HIPCHK(c, hipEventRecord(c->ev_whole, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->aux, c->ev_whole, 0));
  }
  return NEMO_OK;
}
// ... for the entry points that read run 0's graphs only: nothing to do while those are their own
// representatives (run 0 need not be the first run)
static inline int ensure_run0(nemo_ctx *c) {
  if (!c->cs.gd_stale) return NEMO_OK;
  const int32_t r = c->cs.run0;
  if (r < 0 || (c->cs.gd_rep[2 * r] == 2u * r && c->cs.gd_rep[2 * r + 1] == 2u * r + 1u)) return NEMO_OK;
  return ensure_whole(c);
}

// markConditionHolds is deferred for the LDS-tier graphs: nemo_simplify runs
// it fused with the simplification (k_marksimp).  Anything that reads the
// holds flags before that materialises it first (ensure_marked).
static inline int ensure_marked(nemo_ctx *c) {
  if (!c->cs.mark_pending) return NEMO_OK;
  if (int rw = ensure_whole(c)) return rw;  // k_mark walks every tier graph's rows
  const double V = c->cs.tierV, E = c->cs.tierE;
  int rc = timed(c, "k_mark", 8 * E + 13 * V, 2 * E, [&] { nemo::launch_mark(c->cs.dc, false, c->stream); });
  if (rc) return rc;
  c->cs.mark_pending = false;
  c->cs.ms_fused = false;  // k_mark rewrote every graph's flags (holds only)
  return NEMO_OK;
}
